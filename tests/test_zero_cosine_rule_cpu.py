"""The voxel step's rule for direction cosines of zero (trace_step_lazy, csrc/tracer.hpp), restated in numpy float32 (no GPU).

The reference says of an axis whose |cosine| is below 2 tiny that its face is never reached: the face quotient is `huge`
(:1697-1704).  The kernels used to replace the quotient of every axis with |cosine| < 1e-20 by huge and to take the minimum of the
three by a chain of `<` selects.  Now an exact zero is left alone: the quotient the kernels form for it is NaN whatever the
numerator (1 / +-0 = +-inf, and the refinement's fma(-0, inf, 1) is NaN), the minimum is an fmin chain, which ignores NaN, and the
face tests are ordered compares, which are false for NaN as they are for huge.  Cosines with 0 < |d| < 1e-20 keep the old repair --
which, entered by the whole wave, also replaces the NaN of a zero by huge: both forms of the new rule are held against the old one.

Compared: the step, the three face tests and the error test `!(step > 0)`."""
import numpy as np

f32 = np.float32
HUGE = np.finfo(f32).max
TINY = np.finfo(f32).tiny
SLOW = f32(1e-20)


def _quotients(num, d):
    """what the kernels hold before any repair: the correctly rounded quotient (exact_div is IEEE `/`: test_exact_arithmetic_helpers)
    for a cosine the reciprocal reaches, and for +-0 the operations of refined_rcp / exact_div themselves"""
    with np.errstate(all="ignore"):
        q = (num / d).astype(f32)
        zero = d == 0
        r0 = (f32(1.0) / d).astype(f32)                      # v_rcp_f32: +-inf for +-0
        r1 = ((-d * r0 + f32(1.0)) * r0 + r0).astype(f32)    # refined_rcp: -0 * inf is NaN (fused or not)
        q0 = (num * r1).astype(f32)
        q1 = ((-d * q0 + num) * r1 + q0).astype(f32)
        q2 = ((-d * q1 + num) * r1 + q1).astype(f32)
    assert np.isnan(q2[zero]).all()
    return np.where(zero, q2, q)


def _repair(q, num, d):
    """the guarded path: |d| < 1e-20 -> huge, and the IEEE quotient where 2 tiny <= |d|"""
    ad = np.abs(d)
    with np.errstate(all="ignore"):
        ieee = (num / d).astype(f32)
    out = np.where(ad < SLOW, HUGE, q)
    return np.where((ad < SLOW) & (ad >= f32(2.0) * TINY), ieee, out).astype(f32)


def old_rule(num, d):
    st = _repair(_quotients(num, d), num, d)               # (the wave-uniform test only skipped the repair where it changes nothing)
    step = st[:, 0].copy()
    step = np.where(st[:, 1] < step, st[:, 1], step)
    step = np.where(st[:, 2] < step, st[:, 2], step)
    return step, st <= step[:, None], ~(step > 0)


def new_rule(num, d, wave_repairs):
    """wave_repairs: some lane of the wave holds a cosine with 0 < |d| < 1e-20, so every lane runs the repair"""
    st = _quotients(num, d)
    ad = np.abs(d)
    slow = ((ad > 0) & (ad < SLOW)).any(axis=1)
    st = np.where((slow | wave_repairs)[:, None], _repair(st, num, d), st)
    with np.errstate(invalid="ignore"):
        step = np.fmin(np.fmin(st[:, 0], st[:, 1]), st[:, 2])
        return step, st <= step[:, None], ~(step > 0)


def slow_flag(d):
    """Ray::set_direction: the bit patterns shifted left (the sign drops out) less one, as unsigned, so that zero becomes the largest"""
    with np.errstate(over="ignore"):
        bits = ((np.ascontiguousarray(d).view(np.uint32) << np.uint32(1)) - np.uint32(1)).min(axis=1)
        return bits < (np.array(SLOW).view(np.uint32) << np.uint32(1)) - np.uint32(1)


def _inputs():
    rng = np.random.default_rng(5)
    n = 100_000
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    num = (np.where(d >= 0, 1.0, -1.0) * rng.random((n, 3)) * 10.0 ** rng.uniform(-5, 1, (n, 3))).astype(f32)
    # every pattern of one or two axes at +0 or -0
    pats = []
    for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
        for signs in range(1 << len(axes)):
            pats.append([(a, f32(-0.0) if signs >> k & 1 else f32(0.0)) for k, a in enumerate(axes)])
    for k, p in enumerate(pats * 200):
        for a, z in p:
            d[k, a] = z
    at = len(pats) * 200
    # the tiny classes, alone and next to a zero
    for k, t in enumerate((1e-25, -3e-30, 1e-39, -1e-39, 2.0 * float(TINY), 1e-20, 9.99e-21)):
        for a in range(3):
            d[at, a] = f32(t); at += 1
            d[at, a] = f32(t); d[at, (a + 1) % 3] = f32(-0.0 if k & 1 else 0.0); at += 1
    # zero numerators (a start on the face the ray moves towards), on live and on zero axes
    z = slice(at, at + 3000); at += 3000
    num[z] = np.where(rng.random((3000, 3)) < 0.4, f32(0.0), num[z])
    num[z][::2] = np.where(num[z][::2] == 0, f32(-0.0), num[z][::2])
    d[at - 1500:at, 0] = f32(0.0)
    # quotient ties between axes, two and three ways, also next to a zero
    t = slice(at, at + 3000); at += 3000
    d[t] = np.where(d[t] >= 0, f32(0.5), f32(-0.5))
    num[t, 1] = np.abs(num[t, 0]) * np.sign(d[t, 1])
    num[t, 0] = np.abs(num[t, 0]) * np.sign(d[t, 0])
    num[at - 2000:at, 2] = np.abs(num[at - 2000:at, 0]) * np.sign(d[at - 2000:at, 2])
    d[at - 1000:at, 2] = f32(-0.0)
    # wrong-side numerators: a negative step is the tracer's error
    num[at:at + 500, 1] *= f32(-1.0)
    return num, d


def test_new_rule_equals_old_rule():
    num, d = _inputs()
    ad = np.abs(d)
    assert ((d == 0).sum(axis=1) == 1).sum() > 1000 and ((d == 0).sum(axis=1) == 2).sum() > 1000
    assert (np.signbit(d) & (d == 0)).any() and (~np.signbit(d) & (d == 0)).any()
    assert ((ad > 0) & (ad < SLOW)).any() and ((num == 0) & (d == 0)).any() and ((num == 0) & (d != 0)).any()
    step0, hit0, err0 = old_rule(num, d)
    assert (hit0.sum(axis=1) >= 2).sum() > 1000 and err0.sum() > 100 and (~err0).sum() > 90_000
    for wave_repairs in (False, True):
        step, hit, err = new_rule(num, d, np.full(len(d), wave_repairs))
        assert np.array_equal(err, err0)
        assert np.array_equal(step[~err], step0[~err])           # (a step that ends the trace may differ in the sign of its zero)
        assert not np.isnan(step).any() and (step[err] <= 0).all() and (step0[err] <= 0).all()
        assert np.array_equal(hit[~err], hit0[~err])


def test_slow_flag_is_set_by_tiny_cosines_only():
    _, d = _inputs()
    ad = np.abs(d)
    want = ((ad > 0) & (ad < SLOW)).any(axis=1)
    assert want.sum() > 30 and np.array_equal(slow_flag(d), want)
    edge = np.array([[0.0, -0.0, 1.0], [1e-20, 0.0, 1.0], [np.nextafter(SLOW, f32(0)), 0.0, 1.0], [1e-45, 1.0, 0.0], [-1e-45, -0.0, 1.0],
                     [0.0, 0.0, -1.0], [1.0, 0.0, -1e-25]], f32)
    assert list(slow_flag(edge)) == [False, False, True, True, True, False, True]
