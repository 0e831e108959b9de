"""Tabulated gain / RCS patterns on the host (no GPU): rts_pattern_eval against an independent restatement of the semantics in
include/rts_amd.h (RtsPattern), and the validation of malformed descriptors."""
import math

import numpy as np
import pytest


def lerp_ref(s, y, x):
    """piecewise-linear over ascending s, clamped: y_i + t (y_{i+1} - y_i), t = (x - s_i) / (s_{i+1} - s_i)"""
    n = len(s)
    if n == 1 or x <= s[0]:
        return float(y[0])
    if x >= s[-1]:
        return float(y[-1])
    i = int(np.searchsorted(s, x, side="right")) - 1
    t = (x - s[i]) / (s[i + 1] - s[i])
    return float(y[i] + t * (y[i + 1] - y[i]))


def grid_ref(g, u0, du, v0, dv, u, v):
    n_v, n_u = g.shape

    def cell(x, x0, dx, n):
        f = min(max((x - x0) / dx, 0.0), n - 1.0)
        if n < 2:
            return 0, 0, 0.0
        i = min(int(math.floor(f)), n - 2)
        return i, i + 1, f - i
    i, i1, tu = cell(u, u0, du, n_u)
    j, j1, tv = cell(v, v0, dv, n_v)
    a = g[j, i] + tu * (g[j, i1] - g[j, i])
    b = g[j1, i] + tu * (g[j1, i1] - g[j1, i])
    return float(a + tv * (b - a))


def separable_ref(us, uy, vs, vy, scale, abs_u, abs_v, u, v):
    return scale * lerp_ref(us, uy, abs(u) if abs_u else u) * lerp_ref(vs, vy, abs(v) if abs_v else v)


def _axis(rng, n, lo, hi):
    s = np.sort(rng.uniform(lo, hi, n))
    while n > 1 and np.any(np.diff(s) <= 0):
        s = np.sort(rng.uniform(lo, hi, n))
    return s


def _points(rng, lo, hi, samples=None, n=200):
    w = hi - lo
    p = [rng.uniform(lo - 0.5 * w - 1.0, lo), rng.uniform(hi, hi + 0.5 * w + 1.0), rng.uniform(lo, hi, n)]
    if samples is not None:
        p.append(samples)                                      # exactly on the sample abscissae
    return np.concatenate([np.atleast_1d(x) for x in p])


def test_constant_pattern_is_its_scale_exactly(rts):
    for c in (0.0, 1.0, 0.3, 7.25e-3, 1e300):
        out = rts.pattern_eval(rts.Pattern.constant(c), np.linspace(-10, 10, 9), np.linspace(5, -5, 9))
        assert out.tobytes() == np.full(9, c).tobytes()


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("abs_u,abs_v", [(False, False), (True, False), (False, True), (True, True)])
def test_separable_against_restatement(rts, seed, abs_u, abs_v):
    rng = np.random.default_rng(1000 * seed + 2 * abs_u + abs_v)
    n_u = [1, 2, 3, 17, 64, 5][seed]; n_v = [1, 4, 1, 9, 2, 33][seed]
    us = _axis(rng, n_u, -math.pi, math.pi); vs = _axis(rng, n_v, -1.5, 1.5)
    uy = rng.uniform(0.0, 3.0, n_u); vy = rng.uniform(0.0, 2.0, n_v); scale = rng.uniform(0.1, 4.0)
    p = rts.Pattern.separable(us, uy, vs, vy, scale=scale, abs_u=abs_u, abs_v=abs_v)
    pu = _points(rng, us[0], us[-1], us); pv = _points(rng, vs[0], vs[-1], vs)
    m = max(len(pu), len(pv))
    u = np.resize(pu, m); v = np.resize(pv, m)
    rng.shuffle(v)
    got = rts.pattern_eval(p, u, v)
    want = np.array([separable_ref(us, uy, vs, vy, scale, abs_u, abs_v, a, b) for a, b in zip(u, v)])
    tol = 1e-14 * scale * uy.max() * vy.max()
    np.testing.assert_allclose(got, want, rtol=0, atol=tol)
    # the values at the samples themselves (only where the flag does not fold the axis)
    if not abs_u and not abs_v:
        at = rts.pattern_eval(p, us, np.full(n_u, vs[0]))
        np.testing.assert_allclose(at, scale * uy * vy[0], rtol=0, atol=tol)


@pytest.mark.parametrize("seed", range(6))
def test_grid_against_restatement(rts, seed):
    rng = np.random.default_rng(77 + seed)
    n_u = [2, 7, 1, 36, 3, 64][seed]; n_v = [2, 5, 4, 1, 19, 33][seed]
    g = rng.uniform(0.0, 5.0, (n_v, n_u))
    u0, du = rng.uniform(-3.2, -2.0), rng.uniform(0.01, 0.3); v0, dv = rng.uniform(-1.6, -0.5), rng.uniform(0.02, 0.2)
    scale = rng.uniform(0.5, 2.0)
    p = rts.Pattern.grid(g, u0, du, v0, dv, scale=scale)
    ug = u0 + np.arange(n_u) * du; vg = v0 + np.arange(n_v) * dv
    u = _points(rng, ug[0], ug[-1] if n_u > 1 else ug[0] + du, ug); v = _points(rng, vg[0], vg[-1] if n_v > 1 else vg[0] + dv, vg)
    m = max(len(u), len(v)); u = np.resize(u, m); v = np.resize(v, m); rng.shuffle(v)
    got = rts.pattern_eval(p, u, v)
    want = np.array([scale * grid_ref(g, u0, du, v0, dv, a, b) for a, b in zip(u, v)])
    tol = 1e-14 * scale * g.max()
    np.testing.assert_allclose(got, want, rtol=0, atol=tol)
    # on the grid lines: the samples, scaled
    jj, ii = np.meshgrid(np.arange(n_v), np.arange(n_u), indexing="ij")
    on = rts.pattern_eval(p, u0 + ii * du, v0 + jj * dv)
    np.testing.assert_allclose(on, scale * g, rtol=0, atol=tol)
    # clamped: far outside in every direction reads the corner / edge samples
    far = rts.pattern_eval(p, [u0 - 100.0, u0 + 100.0 + n_u * du, u0 - 100.0, u0 + 100.0 + n_u * du],
                           [v0 - 100.0, v0 - 100.0, v0 + 100.0 + n_v * dv, v0 + 100.0 + n_v * dv])
    np.testing.assert_allclose(far, scale * np.array([g[0, 0], g[0, -1], g[-1, 0], g[-1, -1]]), rtol=0, atol=tol)


def test_pattern_eval_matches_wrap_free_arguments(rts):
    """the evaluator takes u, v as given (no wrap inside the pattern): a grid over [-pi, pi) clamps beyond it"""
    g = np.array([[1.0, 2.0, 3.0]])
    p = rts.Pattern.grid(g, -math.pi, math.pi, 0.0, 1.0)
    assert rts.pattern_eval(p, [4.0], [0.0])[0] == 3.0 and rts.pattern_eval(p, [-4.0], [0.0])[0] == 1.0


def _sep(rts, **kw):
    a = dict(u_samples=[0.0, 1.0], u_values=[1.0, 2.0], v_samples=[0.0, 1.0], v_values=[1.0, 1.0])
    a.update(kw)
    return rts.Pattern.separable(a["u_samples"], a["u_values"], a["v_samples"], a["v_values"])


def _malformed(rts):
    from rts_amd import _lib as L
    nan = float("nan")
    out = {
        "duplicate samples": _sep(rts, u_samples=[0.0, 0.0], u_values=[1.0, 1.0]),
        "descending samples": _sep(rts, v_samples=[1.0, 0.0]),
        "nan sample": _sep(rts, u_samples=[0.0, nan]),
        "inf sample": _sep(rts, u_samples=[0.0, float("inf")]),
        "nan value": _sep(rts, u_values=[1.0, nan]),
        "negative value": _sep(rts, v_values=[1.0, -1e-300]),
        "n = 0": _sep(rts, u_samples=[], u_values=[]),
        "nan grid": rts.Pattern.grid([[1.0, nan]], 0.0, 1.0, 0.0, 1.0),
        "negative grid": rts.Pattern.grid([[1.0, -2.0]], 0.0, 1.0, 0.0, 1.0),
        "du = 0": rts.Pattern.grid([[1.0, 2.0]], 0.0, 0.0, 0.0, 1.0),
        "du < 0": rts.Pattern.grid([[1.0, 2.0]], 0.0, -1.0, 0.0, 1.0),
        "dv = 0": rts.Pattern.grid([[1.0, 2.0]], 0.0, 1.0, 0.0, 0.0),
        "nan origin": rts.Pattern.grid([[1.0, 2.0]], nan, 1.0, 0.0, 1.0),
        "empty grid": rts.Pattern.grid(np.zeros((0, 3)), 0.0, 1.0, 0.0, 1.0),
        "negative scale": rts.Pattern.constant(-1.0),
        "nan scale": rts.Pattern.constant(nan),
    }
    d = rts.Pattern.constant(1.0).desc(); d.kind = 3; out["unknown kind"] = d
    d = _sep(rts).desc(); d.flags = 4; out["unknown flag"] = d
    d = rts.Pattern.constant(1.0).desc(); d.flags = L.RTS_PATTERN_ABS_U; out["flag on a constant"] = d
    d = rts.Pattern.grid([[1.0, 2.0]], 0.0, 1.0, 0.0, 1.0).desc(); d.flags = L.RTS_PATTERN_ABS_V; out["flag on a grid"] = d
    d = rts.Pattern.constant(1.0).desc(); d.reserved[1] = 1; out["reserved field"] = d
    for f in ("u_samples", "u_values", "v_samples", "v_values"):
        d = _sep(rts).desc(); setattr(d, f, None); out["null " + f] = d
    d = rts.Pattern.grid([[1.0, 2.0]], 0.0, 1.0, 0.0, 1.0).desc(); d.grid = None; out["null grid"] = d
    d = _sep(rts).desc(); d.n_u = L.RTS_PATTERN_MAX_AXIS + 1; out["oversize axis"] = d           # (rejected before the arrays are read)
    d = rts.Pattern.grid([[1.0, 2.0]], 0.0, 1.0, 0.0, 1.0).desc(); d.n_u = 4096; d.n_v = 4096; out["oversize grid"] = d
    return out


def test_malformed_patterns_are_rejected(rts):
    from rts_amd import _lib as L
    import ctypes as C
    u = np.zeros(3); v = np.zeros(3); out = np.full(3, 7.0)
    for name, p in _malformed(rts).items():
        d = p if isinstance(p, L.RtsPattern) else p.desc()
        rc = L.lib().rts_pattern_eval(C.byref(d), L.ptr(u), L.ptr(v), 3, L.ptr(out))
        assert rc == L.RTS_ERR_INVALID, name
        assert out.tobytes() == np.full(3, 7.0).tobytes(), name          # nothing written
        with pytest.raises(L.RtsError):
            rts.pattern_eval(p, u, v)
    assert L.lib().rts_pattern_eval(None, L.ptr(u), L.ptr(v), 3, L.ptr(out)) == L.RTS_ERR_INVALID
    good = rts.Pattern.constant(2.0).desc()
    assert L.lib().rts_pattern_eval(C.byref(good), None, L.ptr(v), 3, L.ptr(out)) == L.RTS_ERR_INVALID
    assert L.lib().rts_pattern_eval(C.byref(good), L.ptr(u), L.ptr(v), 3, None) == L.RTS_ERR_INVALID
    assert L.lib().rts_pattern_eval(C.byref(good), None, None, 0, None) == L.RTS_OK


def test_pattern_entry_points_fail_without_a_handle(rts):
    from rts_amd import _lib as L
    import ctypes as C
    p = rts.Pattern.constant(1.0).desc()
    assert L.lib().rts_set_patterns(None, C.byref(p), None, 0, None, 0) == L.RTS_ERR_INVALID
    q = L.RtsPatternPulse(0.03, 1e10, 299792458.0, None, None)
    assert L.lib().rts_finalise_patterns(None, C.byref(q)) == L.RTS_ERR_INVALID
    assert L.lib().rts_trace_pulse_end_patterns(None, C.byref(q), -1, 0) == L.RTS_ERR_INVALID
