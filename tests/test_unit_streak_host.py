"""The unit-step form of the far-field streak's fixed-quadrant loop (kerr_rk4_streak, lt_device.hpp) drops
the loop's per-step range test `lam <= lam_limit`, lam_limit = lambda_max - h_base, after ONE test on the state the call
starts from: every lane at least cap + 1 below the limit, cap being the call's attempt cap.  The recurrence is restated
here in numpy float32 -- its add and subtract are the device's v_add_f32 / v_sub_f32 roundings -- and run for cap
attempts from starting values on both sides of that bound: wherever the hoisted test holds, the per-step test it
replaces must hold on every attempt of the call.  Two statements of the hoisted test are held to that: the margin taken
off the limit, lam_0 <= lam_limit - (cap + 1), for base steps 1 and 0.5, and the form the kernel evaluates,
lam_0 + (cap + 1) <= lambda_max - 1, which it only reaches with a base step of exactly 1 and lambda_max <= 2^13.  No GPU."""
import numpy as np
import pytest

F = np.float32
CAPS = (64, 384)
LAMBDA_MAX = (5000.0, 8192.0, 4999.7, 1000.3, 500.0, 449.95, 150.0, 100.5, 66.0, 65.5, 60.5, 37.25)


def neighbours(x, n):
    """x and its n float32 neighbours on either side"""
    out, lo, hi = [F(x)], F(x), F(x)
    for _ in range(n):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return out


def starts(lam_max, hb, cap):
    """Starting values of a call: next to the bound on either side (every float32 within 40 ulp, and the bound moved by up
    to two base steps), what a ray really carries -- sums of the tracer's step sizes, accumulated in float32 -- and
    values spread over the whole range."""
    bound = F(F(lam_max) - F(hb)) - F(cap + 1)
    vals = []
    for d in np.arange(-2.0, 2.01, 0.125):
        vals += neighbours(bound + F(d), 40)
    rng = np.random.default_rng(int(cap * 1000 + lam_max))
    acc = np.zeros(512, dtype=F)
    for _ in range(400):   # a ray's lam: steps of 1, 0.5, 0.25, 0.2, 0.1, 0.08, 0.05, 0.03 and halved retries, added one by one
        acc = (acc + rng.choice(np.array([1, 1, 1, 0.5, 0.25, 0.2, 0.1, 0.08, 0.05, 0.03, 0.025, 0.0125], dtype=F), size=acc.size)).astype(F)
        vals += list(acc[::64])
    vals += list((bound + acc - F(100.0)).astype(F)) + list(rng.uniform(0.0, lam_max, 2000).astype(F))
    v = np.array(vals, dtype=F)
    return v[(v >= 0) & np.isfinite(v)]


def per_step_tests(lam0, hb, cap, lam_max):
    """The loop's own test on each of the cap attempts of a call that nothing else ends: (cap, n) bool."""
    lam_limit = F(lam_max) - F(hb)
    assert lam_limit.dtype == F
    lam, out = lam0.copy(), []
    for _ in range(cap):
        out.append(lam <= lam_limit)
        lam = (lam + F(hb)).astype(F)
    return np.array(out)


def hoisted_off_the_limit(lam0, hb, cap, lam_max):
    return lam0 <= (F(lam_max) - F(hb)) - F(cap + 1)


def hoisted_as_the_kernel_does(lam0, hb, cap, lam_max):
    # make_kerr: unit_lam = lambda_max - 1 in float32, -inf beyond 2^13; kerr_rk4_streak: hb == 1, the margin added to lam
    unit_lam = F(lam_max) - F(1) if F(lam_max) <= F(8192) else F(-np.inf)
    return (F(hb) == F(1)) & (cap <= 4096) & ((lam0 + F(cap + 1)).astype(F) <= unit_lam)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("hb", (1.0, 0.5))
@pytest.mark.parametrize("hoisted", (hoisted_off_the_limit, hoisted_as_the_kernel_does))
def test_the_hoisted_test_implies_the_per_step_test_on_every_attempt(hoisted, hb, cap):
    seen_true = seen_false = seen_fail = 0
    for lam_max in LAMBDA_MAX:
        lam0 = starts(lam_max, hb, cap)
        step = per_step_tests(lam0, hb, cap, lam_max)
        ok = hoisted(lam0, hb, cap, lam_max)
        bad = ok & ~step.all(axis=0)
        assert not bad.any(), (lam_max, lam0[bad][:5], np.argmin(step[:, bad], axis=0)[:5])
        seen_true += int(ok.sum())
        seen_false += int((~ok).sum())
        seen_fail += int((~step.all(axis=0)).sum())
    # both sides of the bound were reached, and so were calls in which the per-step test fails
    assert seen_false > 0 and seen_fail > 0
    if hoisted is hoisted_as_the_kernel_does and hb != 1.0:
        assert seen_true == 0   # the kernel takes the form with a base step of exactly 1 only
    else:
        assert seen_true > 0


@pytest.mark.parametrize("cap", CAPS)
def test_the_margin_is_not_idle_at_a_unit_step(cap):
    # the + 1 of the margin is what the rounding of cap additions may use up; it is small: a call that starts two steps
    # above the bound runs into the per-step test before it ends
    for lam_max in (5000.0, 8192.0, 500.0):
        bound = (F(lam_max) - F(1)) - F(cap + 1)
        lam0 = np.array([bound + F(2.5)], dtype=F)
        assert not hoisted_as_the_kernel_does(lam0, 1.0, cap, lam_max)[0]
        assert not per_step_tests(lam0, 1.0, cap, lam_max).all()


def test_the_kernel_never_takes_the_form_beyond_the_range_the_margin_is_proved_for():
    lam0 = np.array([0.0, 1.0, 100.0], dtype=F)
    for lam_max in (8192.5, 1e4, 1e6, 2.0 ** 24, 1e9):
        assert not hoisted_as_the_kernel_does(lam0, 1.0, 64, lam_max).any()
