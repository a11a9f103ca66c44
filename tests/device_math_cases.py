"""Arguments, extended-precision references and the checks of the packet loop's own math (mc_device.hip.h: sqrt_nonneg,
sqrt_fast_nonneg, log_pos, tau_of_draw, f64_to_i32_sat, sad_plus1_u32, sincos_pi, az_sector_certain, az_sector, cdapres_pi,
rotation, stokes_rotation, stokes_apply, hg_draw), shared by tests/test_device_math_gpu.py (the device's instruction
sequences, mcgpu_probe_math) and tests/test_device_math_emulated.py (the host branches of the same functions in the one-lane
emulation, tests/emu/emu_math.cpp -- what the host tail computes).

A `probe` is a callable probe(kind, *rows) -> float64 [n_out, n] (Engine.probe_math or the emulation's wrapper); every
check_* takes one, asserts, and returns the figures it measured.  The references are written from the mathematical
definitions the comments of mc_device.hip.h give, with >= 63 mantissa bits (numpy.longdouble for the arrays, mpmath for a
handful of values); none calls the oracle or the library.  EPS is 2^-53."""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
TINY_REAL = float(np.finfo(np.float32).tiny)
TINY_DP = float(np.finfo(np.float64).tiny)
W0_THRESHOLD = float(np.float32(0.999999))      # cdapres: (double)0.999999f


def require_extended():
    assert np.finfo(LD).nmant >= 63, "numpy.longdouble has %d mantissa bits here: the references need >= 63" % np.finfo(LD).nmant


def pi_ld():
    require_extended()
    return LD("3.14159265358979323846264338327950288419716939937510")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def ulp_distance(a, b):
    """units in the last place between non-negative finite doubles"""
    return np.abs(_bits(a) - _bits(b))


def sincospi_ld(x):
    """sin(pi x), cos(pi x) in extended precision, the argument reduced exactly (x - rint(x) is exact in float64)"""
    x = np.asarray(x, np.float64)
    n = np.rint(x)
    r = (x - n).astype(LD)
    sgn = (1.0 - 2.0 * np.mod(n, 2.0)).astype(LD)
    return np.sin(pi_ld() * r) * sgn, np.cos(pi_ld() * r) * sgn


# ---- sqrt_nonneg, sqrt_fast_nonneg --------------------------------------------------------------------------------------
@functools.lru_cache(None)
def sqrt_inputs():
    """0, 2^-767 and (1e6 AU)^2; 2e5 random mantissas per exponent parity over 2^-766 .. 2^80; exact squares with their
    two neighbours; 2e5 near-midpoint arguments: t = q^2 + q = (q + 1/2)^2 - 1/4 for integers q in [2^52, 2^53), rounded to
    53 bits downwards and upwards, scaled by even and by odd powers of two."""
    rng = np.random.default_rng(20240501)
    parts = [np.array([0.0, 2.0 ** -767, 1.0e12])]
    for parity in (0, 1):
        e = 2 * rng.integers(-383, 40, 200000) + parity
        parts.append(np.ldexp(1.0 + rng.random(200000), e))
    k = rng.integers(1, 2 ** 26, 20000).astype(np.float64)
    sq = np.ldexp(k * k, 2 * rng.integers(-350, 10, k.size))          # (k^2 < 2^52: exact)
    parts += [sq, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf)]
    q = [int(v) for v in rng.integers(2 ** 52, 2 ** 53, 100000)]
    lo, sh = np.empty(len(q)), np.empty(len(q), np.int64)
    for i, v in enumerate(q):
        t = v * v + v
        s = t.bit_length() - 53
        lo[i], sh[i] = float(t >> s), s
    scale = rng.integers(-700, 70, len(q)) - 105                          # even and odd alike
    parts += [np.ldexp(lo, sh + scale), np.ldexp(lo + 1.0, sh + scale)]
    x = np.concatenate(parts)
    assert x.min() == 0.0 and np.all((x == 0.0) | (x >= 2.0 ** -767)) and x.max() < 2.0 ** 81
    return x


def check_sqrt_nonneg(probe):
    """bit equality with numpy's sqrt (IEEE: correctly rounded)"""
    x = sqrt_inputs()
    got, ref = probe("sqrt_nonneg", x)[0], np.sqrt(x)
    bad = _bits(got) != _bits(ref)
    fig = dict(n=x.size, n_differ=int(bad.sum()))
    if bad.any():
        with np.errstate(invalid="ignore"):
            fig["max_ulp"] = int(ulp_distance(got[bad], ref[bad]).max())
        fig["first"] = [(float(a), float(b), float(c)) for a, b, c in zip(x[bad][:5], got[bad][:5], ref[bad][:5])]
        fig["range"] = (float(x[bad].min()), float(x[bad].max()))
    print("sqrt_nonneg:", fig)
    assert not bad.any(), fig
    return fig


SQRT_FAST_MAX_ULP = 4     # the comment's "few"


def check_sqrt_fast_nonneg(probe):
    x = sqrt_inputs()
    got, ref = probe("sqrt_fast_nonneg", x)[0], np.sqrt(x)
    assert np.all(_bits(got[x == 0.0]) == 0), "exactly +0 at 0"
    assert np.all(got >= 0.0) and np.all(np.isfinite(got))
    d = ulp_distance(got, ref)
    fig = dict(n=x.size, max_ulp=int(d.max()), n_differ=int((d > 0).sum()), worst_x=float(x[d.argmax()]))
    print("sqrt_fast_nonneg:", fig)
    assert d.max() <= SQRT_FAST_MAX_ULP, fig
    return fig


# ---- log_pos, tau_of_draw ---------------------------------------------------------------------------------------------
# The project's claim (mc_device.hip.h::log_pos).  It was 4e-16; the device measured 4.61e-16 at x = 1.3171283928715891 (11
# of the 1.1e6 arguments below beyond 4e-16) and 4.23e-16 over the 2^24 optical depths (draw 3772363): the comment now
# states the measured bound plus one ulp, and tau_of_draw, which IS -log_pos(1 - rand) of an exact argument, follows it.
LOG_POS_REL = 7.0e-16


@functools.lru_cache(None)
def log_inputs():
    """1e6 arguments log-uniform over [TINY_DP, 1e300]; the mantissa boundary the code branches on (m within 3 ulp of
    0.70710678118654752, at several exponents); 1 and its neighbours; 2^k and its neighbours, k = -1022 .. 1023 (normal
    numbers only); 1e5 arguments in [0.5, 2]."""
    rng = np.random.default_rng(20240502)
    parts = [np.exp(rng.uniform(np.log(TINY_DP), np.log(1.0e300), 1000000)).clip(TINY_DP, 1.0e300)]
    m = [0.70710678118654752]
    for _ in range(3):
        m = [np.nextafter(m[0], 0.0)] + m + [np.nextafter(m[-1], 1.0)]
    parts.append(np.array([np.ldexp(v, k) for v in m for k in (-1021, -500, -1, 0, 1, 2, 500, 1024)]))
    parts.append(np.array([1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)]))
    p = np.ldexp(1.0, np.arange(-1022, 1024))
    parts += [p, np.nextafter(p, np.inf), np.nextafter(p[1:], 0.0)]
    parts.append(rng.uniform(0.5, 2.0, 100000))
    x = np.concatenate(parts)
    assert np.all(x >= TINY_DP) and np.all(np.isfinite(x))
    return x


def check_log_pos(probe):
    require_extended()
    x = log_inputs()
    got = probe("log_pos", x)[0]
    ref = np.log(x.astype(LD))
    one = x == 1.0
    assert np.all(got[one] == 0.0), "log_pos(1) = 0"
    rel = np.abs((got[~one].astype(LD) - ref[~one]) / ref[~one]).astype(np.float64)
    w = rel.argmax()
    fig = dict(n=x.size, max_rel=float(rel.max()), worst_x=float(x[~one][w]), n_over=int((rel > LOG_POS_REL).sum()))
    print("log_pos:", fig)
    assert rel.max() <= LOG_POS_REL, fig
    return fig


def check_tau_of_draw(probe):
    """every default-real draw k / 2^24: -log1p(-r) to LOG_POS_REL above the branch point 1e-6f, (double)rand below it,
    non-decreasing in k throughout"""
    require_extended()
    n = 1 << 24
    r = np.arange(n, dtype=np.float64) / n
    got = probe("tau_of_draw", r)[0]
    above = r.astype(np.float32) > np.float32(1.0e-6)
    assert above[17] and not above[16]          # (the branch point lies between the draws 16 and 17 / 2^24)
    assert np.array_equal(got[~above], r[~above])
    assert np.all(np.diff(got) >= 0.0), "tau_of_draw must not decrease with the draw"
    worst, where = 0.0, -1
    for a in range(0, n, 1 << 20):
        sl = slice(a, a + (1 << 20))
        sel = above[sl]
        ref = -np.log1p(-(r[sl][sel].astype(LD)))
        rel = np.abs((got[sl][sel].astype(LD) - ref) / ref).astype(np.float64)
        if rel.max() > worst:
            worst, where = float(rel.max()), a + int(np.flatnonzero(sel)[rel.argmax()])
    fig = dict(n=n, max_rel=worst, worst_draw=where)
    print("tau_of_draw:", fig)
    assert worst <= LOG_POS_REL, fig
    return fig


# ---- f64_to_i32_sat, sad_plus1_u32 ------------------------------------------------------------------------------------
def check_f64_to_i32_sat(probe):
    rng = np.random.default_rng(20240503)
    i31 = 2147483647.0
    x = np.concatenate([np.array([0.0, -0.0, 0.5, 1.0 - EPS, i31, np.nextafter(i31, 0.0), np.nextafter(i31, np.inf), i31 - 1.0,
                                  i31 - 0.5, 2.0 ** 31, 2.0 ** 32, 2.0 ** 53, 1.0e300, np.inf, np.nan]),
                        rng.uniform(0.0, 2.0 ** 32, 100000)])
    want = np.zeros(x.size, np.int64)          # a NaN gives 0
    num = ~np.isnan(x)
    big = np.zeros(x.size, bool)
    big[num] = x[num] >= i31
    want[big] = 2147483647
    small = num & ~big
    want[small] = np.trunc(x[small]).astype(np.int64)
    got = probe("f64_to_i32_sat", x)[0]
    assert np.array_equal(got, want.astype(np.float64)), (x[got != want][:8], got[got != want][:8])


def check_sad_plus1_u32(probe):
    rng = np.random.default_rng(20240504)
    s = np.array([0, 1, 2, 3, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2], np.int64)
    a = np.concatenate([np.repeat(s, s.size), rng.integers(0, 2 ** 32 - 1, 100000)])
    b = np.concatenate([np.tile(s, s.size), rng.integers(0, 2 ** 32 - 1, 100000)])
    assert np.abs(a - b).max() < 2 ** 32 - 1
    got = probe("sad_plus1_u32", a.astype(np.float64), b.astype(np.float64))[0]
    assert np.array_equal(got, (np.abs(a - b) + 1).astype(np.float64))


# ---- sincos_pi --------------------------------------------------------------------------------------------------------
SINCOS_PI_ABS = np.pi * EPS + 2.0 * EPS    # the rounding of the product pi x (|x| <= 2: 2 eps pi / 2 ... conceded) + one ulp at 1


@functools.lru_cache(None)
def _sin_table():
    """sin(pi j / 2^23), j = 0 .. 2^22, in extended precision: every sin(pi x) and cos(pi x) of a multiple x of 2^-23 is
    +- one of these (the symmetries are index arithmetic, exact)"""
    return np.sin(pi_ld() * (np.arange((1 << 22) + 1, dtype=np.float64) / (1 << 23)).astype(LD))


def _sin_pi_of_multiple(m):
    """sin(pi m / 2^23) for integers m, from the table"""
    T = _sin_table()
    m = np.mod(m, 1 << 24)
    neg = m >= (1 << 23)
    m = np.where(neg, m - (1 << 23), m)
    m = np.where(m > (1 << 22), (1 << 23) - m, m)
    v = T[m]
    return np.where(neg, -v, v)


SINCOS_RANGES = {"2r-1": -(1 << 23), "2r": 0}     # x = m / 2^23 for m from this on, 2^24 of them


def check_sincos_pi(probe, which):
    """every azimuth the packet loop forms: x = 2 rand - 1 or x = 2 rand (`which`) for all 2^24 draws, one launch"""
    require_extended()
    n = 1 << 24
    m = np.arange(n, dtype=np.int64) + SINCOS_RANGES[which]
    s, c = probe("sincos_pi", m.astype(np.float64) / (1 << 23))
    es = ec = 0.0
    for a in range(0, n, 1 << 21):
        sl = slice(a, a + (1 << 21))
        es = max(es, float(np.abs(s[sl].astype(LD) - _sin_pi_of_multiple(m[sl])).max()))
        ec = max(ec, float(np.abs(c[sl].astype(LD) - _sin_pi_of_multiple(m[sl] + (1 << 22))).max()))
    print("sincos_pi, x = %s: max |s - sin| %.4g, |c - cos| %.4g, bound %.4g" % (which, es, ec, SINCOS_PI_ABS))
    assert es <= SINCOS_PI_ABS and ec <= SINCOS_PI_ABS, (which, es, ec)
    return es, ec


def check_sincos_pi_exact_values(probe):
    """The device's sincospi only: it reduces its argument exactly, so the representable values come out exactly, and next
    to a zero (x = 2 - 2^-23, the largest 2 rand) the sine keeps its relative accuracy -- 4 eps: two ulp of the routine's
    polynomial -- which no product pi * x could."""
    require_extended()
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.0 - 2.0 ** -23])
    s, c = probe("sincos_pi", x)
    assert np.array_equal(s[:6], [0.0, 1.0, -1.0, 0.0, 0.0, -1.0]) and np.array_equal(c[:6], [1.0, 0.0, 0.0, -1.0, -1.0, 0.0])
    s_ref, c_ref = -_sin_table()[1], _sin_pi_of_multiple(np.array([(1 << 24) - 1 + (1 << 22)]))[0]
    assert abs((LD(s[6]) - s_ref) / s_ref) <= 4.0 * EPS and abs(LD(c[6]) - c_ref) <= 2.0 * EPS, (s[6], c[6])


# ---- az_sector_certain, az_sector -------------------------------------------------------------------------------------
AZ_N = (1, 2, 3, 72, 128)
AZ_R = (1.0e-3, 1.0, 300.0, 1.0e4)


def az_delta(n_az):
    return 2.0e-6 * n_az + 1.0e-5


@functools.lru_cache(None)
def az_inputs():
    """every sector edge j / n_az at the offsets f (in sector widths) of the issue, at four radii; then the axes, the four
    diagonals, y = -0.0 and the origin.  Returns x, y, n_az, f (NaN for the special points)."""
    xs, ys, ns, fs = [], [], [], []
    for n_az in AZ_N:
        d = az_delta(n_az)
        for f in (1e-9, -1e-9, 0.5 * d, -0.5 * d, 0.9 * d, -0.9 * d, 1.1 * d, -1.1 * d, 2 * d, -2 * d, 8 * d, -8 * d, 0.5):
            for r in AZ_R:
                ang = 2.0 * np.pi * (np.arange(n_az) + f) / n_az
                xs.append(r * np.cos(ang)); ys.append(r * np.sin(ang))
                ns.append(np.full(n_az, n_az)); fs.append(np.full(n_az, f))
        for r in AZ_R:
            sp = np.array([(r, 0.0), (0.0, r), (-r, 0.0), (0.0, -r), (r, r), (-r, r), (-r, -r), (r, -r), (r, -0.0), (-r, -0.0)])
            xs.append(sp[:, 0]); ys.append(sp[:, 1]); ns.append(np.full(len(sp), n_az)); fs.append(np.full(len(sp), np.nan))
        xs.append(np.array([0.0])); ys.append(np.array([0.0])); ns.append(np.array([n_az])); fs.append(np.array([np.nan]))
    return tuple(np.concatenate(v) for v in (xs, ys, ns, fs))


def az_quotient_ld(x, y, n_az):
    """phi / (2 pi) n_az with phi = modulo(atan2(y, x), 2 pi), in extended precision"""
    two_pi = 2 * pi_ld()
    a = np.arctan2(y.astype(LD), x.astype(LD))
    phi = a - np.floor(a / two_pi) * two_pi
    return phi / two_pi * n_az.astype(LD)


def az_sector_f64(x, y, n_az, recip_form):
    """the reference's two spellings in float64 (cylindrical_grid.f90:1125 and :405)"""
    a = np.arctan2(y, x)
    phi = a - np.floor(a / (2 * np.pi)) * (2 * np.pi)
    nf = n_az.astype(np.float32).astype(np.float64)
    q = phi * (1.0 / (2.0 * np.pi)) * nf if recip_form else phi / (2 * np.pi) * nf
    k = np.floor(q).astype(np.int64) + 1
    return np.where(k == n_az + 1, n_az, k)


def check_az_sector(probe):
    require_extended()
    x, y, n_az, f = az_inputs()
    nd = n_az.astype(np.float64)
    q = az_quotient_ld(x, y, n_az)
    k_true = np.minimum(np.floor(q).astype(np.int64) + 1, n_az)
    k, certain = probe("az_sector_certain", x, y, nd)
    certain = certain != 0.0
    origin = (x == 0.0) & (y == 0.0)
    assert not certain[origin].any(), "no certain answer at the origin"
    # the claim: wherever the fast path answers, its sector is the true one
    wrong = certain & (k != k_true)
    assert not wrong.any(), (x[wrong][:5], y[wrong][:5], n_az[wrong][:5], f[wrong][:5], k[wrong][:5], k_true[wrong][:5])
    # the error bound is delta / 4: within delta / 2 of an edge the fast path cannot answer, at 2 delta and beyond it must
    # (else the test above would hold of a fast path that never answers)
    d = np.array([az_delta(n) for n in n_az])
    assert not certain[np.abs(f) <= 0.5 * d + 1e-12].any()
    assert certain[np.abs(f) >= 2.0 * d - 1e-12].all()
    fig = dict(n=x.size, n_certain=int(certain.sum()), certain_at_1_1_delta=int(certain[np.isclose(np.abs(f), 1.1 * d)].sum()),
               certain_at_0_9_delta=int(certain[np.isclose(np.abs(f), 0.9 * d)].sum()))
    # az_sector: the float64 statement of the reference's two spellings.  The offsets are >= 1e-9 of a sector from an edge,
    # far above an arctangent's last bit: the statement alone decides them.  An axis or a diagonal that IS an edge (extended
    # quotient within 1e-12 of an integer) is decided by that last bit: either neighbouring sector is accepted there -- but
    # for the angle 0, whose arctangent is exact.
    k2 = probe("az_sector", x, y, nd)
    frac = (q - np.floor(q + 0.5)).astype(np.float64)
    on_edge = np.isnan(f) & (np.abs(frac) < 1e-12) & ~((y == 0.0) & (x >= 0.0))
    assert not on_edge[~np.isnan(f)].any() and np.abs(frac[~np.isnan(f)]).min() > 0.5e-9
    for row, recip in ((0, False), (1, True)):
        want = az_sector_f64(x, y, n_az, recip)
        ok = k2[row] == want
        below = np.where(np.floor(q + 0.5).astype(np.int64) == 0, n_az, np.floor(q + 0.5).astype(np.int64))
        above = np.minimum(np.floor(q + 0.5).astype(np.int64) + 1, n_az)
        ok |= on_edge & ((k2[row] == below) | (k2[row] == above))
        assert ok.all(), (recip, x[~ok][:5], y[~ok][:5], n_az[~ok][:5], k2[row][~ok][:5], want[~ok][:5])
    fig["n_on_edge"] = int(on_edge.sum())
    print("az_sector:", fig)
    return fig


# ---- cdapres_pi -------------------------------------------------------------------------------------------------------
def _unit_from_w(w, alpha):
    """(u, v, w) of unit length to the last place: the horizontal part from sqrt(1 - w^2) in extended precision"""
    s = np.sqrt(1 - w.astype(LD) ** 2)
    return (s * np.cos(alpha.astype(LD))).astype(np.float64), (s * np.sin(alpha.astype(LD))).astype(np.float64), w


@functools.lru_cache(None)
def cdapres_inputs():
    """Unit vectors k0 with |w0| on both sides of (double)0.999999f and at it, w0 = +-1, on the axes and at random; cospsi
    in {+-1, 0, +-(1 - 2^-53)}, the loop's own isotropic cosines 2 rand - 1 (multiples of 2^-23) and random doubles in
    [-0.99, 0.99] (a double next to +-1 loses sqrt(1 - cospsi^2) to the rounding of cospsi^2 in ANY evaluation without a
    fused multiply-add -- 2^-55 / sin(psi) -- which is no property of this routine: the loop's cosines are default reals'
    images or HG's, tested apart); the azimuth over 2 rand - 1."""
    rng = np.random.default_rng(20240505)
    t = W0_THRESHOLD
    w = np.array([0.0, 0.3, -0.7, 0.999, 0.9999999, -0.9999999, 1.0, -1.0, t, np.nextafter(t, 0.0), np.nextafter(t, 2.0),
                  -t, -np.nextafter(t, 0.0), -np.nextafter(t, 2.0)])
    w = np.concatenate([w, rng.uniform(-1.0, 1.0, 50)])
    alpha = np.array([0.0, 0.7, 2.1, 4.0])
    W, A = [v.ravel() for v in np.meshgrid(w, alpha, indexing="ij")]
    u0, v0, w0 = _unit_from_w(W, A)
    axes = np.array([(1.0, 0, 0), (0, 1.0, 0), (-1.0, 0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)])
    u0, v0, w0 = np.concatenate([u0, axes[:, 0]]), np.concatenate([v0, axes[:, 1]]), np.concatenate([w0, axes[:, 2]])
    r24 = lambda k: rng.integers(0, 1 << 24, k).astype(np.float64) / (1 << 24)
    c = np.concatenate([[1.0, -1.0, 0.0, 1.0 - EPS, -(1.0 - EPS)], 2.0 * r24(40) - 1.0, rng.uniform(-0.99, 0.99, 20)])
    phi = 2.0 * np.concatenate([[0.0, 0.5, 0.25, 1.0 - 2.0 ** -24], r24(6)]) - 1.0
    I, C_, P = [v.ravel() for v in np.meshgrid(np.arange(u0.size), c, phi, indexing="ij")]
    return C_, P, u0[I], v0[I], w0[I]


def check_cdapres_pi(probe):
    require_extended()
    c, phi, u0, v0, w0 = cdapres_inputs()
    got = probe("cdapres_pi", c, phi, u0, v0, w0)
    cl, ul, vl, wl = (v.astype(LD) for v in (c, u0, v0, w0))
    sphi, cphi = sincospi_ld(phi)
    spsi = np.sqrt(1 - cl * cl)
    a, b = spsi * cphi, spsi * sphi
    gen = np.abs(w0) <= W0_THRESHOLD
    with np.errstate(divide="ignore", invalid="ignore"):
        cc = np.sqrt(1 - wl * wl)
        ref = [np.where(gen, (a * wl * ul - b * vl) / cc + cl * ul, a), np.where(gen, (a * wl * vl + b * ul) / cc + cl * vl, b),
               np.where(gen, cl * wl - a * cc, cl)]
        # 16 eps max(1, 1 / sqrt(1 - w0^2)): the division's amplification; the branch next to the pole does not divide
        tol = np.where(gen, 16.0 * EPS * np.maximum(1.0, (1 / cc).astype(np.float64)), 16.0 * EPS)
    err = np.max([np.abs(g.astype(LD) - r).astype(np.float64) for g, r in zip(got, ref)], axis=0)
    w = (err / tol).argmax()
    fig = dict(n=c.size, max_err_over_tol=float((err / tol).max()), worst=(float(c[w]), float(phi[w]), float(w0[w])))
    print("cdapres_pi:", fig)
    assert np.all(err <= tol), fig
    away = np.abs(w0) <= 0.999
    norm = np.sqrt(got[0] ** 2 + got[1] ** 2 + got[2] ** 2)
    dot = got[0] * u0 + got[1] * v0 + got[2] * w0
    assert np.all(np.abs(norm[away] - 1.0) <= tol[away]) and np.all(np.abs(dot[away] - c[away]) <= tol[away])
    return fig


# ---- rotation, stokes_rotation, stokes_apply --------------------------------------------------------------------------
def rotation_literal(xi, yi, zi, u1, v1, w1, real=LD):
    """rotation (utils.f90:553-601) as the reference spells it: theta = atan2(v1, u1), cos(theta), sin(theta)"""
    xi, yi, zi, ul, vl, wl = (np.asarray(v, np.float64).astype(real) for v in (xi, yi, zi, u1, v1, w1))
    theta = np.arctan2(vl, ul)
    b1 = w1 > 0.999999999
    b2 = ~b1 & (np.abs(u1) < TINY_REAL)
    one, zero = np.ones_like(xi), np.zeros_like(xi)
    cost = np.where(b1, one, np.where(b2, zero, np.cos(theta)))
    sint = np.where(b1, zero, np.where(b2, one, np.sin(theta)))
    sing = np.where(b1, zero, np.sqrt(np.maximum(1 - wl * wl, 0)))
    prod = cost * xi + sint * yi
    return sing * prod + wl * zi, cost * yi - sint * xi, sing * zi - wl * prod


@functools.lru_cache(None)
def rotation_inputs():
    """All three branches: w1 > 0.999999999 (1, 1 - 1e-10, the next double above the threshold); |u1| < tiny (u1 = 0, 1e-39;
    v1 of either sign; w1 = -1); the general one (random, v1 = 0 with u1 of either sign, w1 = 0.999999999 itself)."""
    rng = np.random.default_rng(20240506)
    k1 = [(0.0, 0.0, 1.0), (np.sqrt(1 - (1 - 1e-10) ** 2), 0.0, 1 - 1e-10), (0.0, 0.0, -1.0)]
    wt = 0.999999999
    for w in (np.nextafter(wt, 2.0), wt):
        s = float(np.sqrt(1 - LD(w) ** 2))
        k1 += [(s * 0.6, s * 0.8, w)]
    for w in (0.5, -0.3, 0.999, 0.0):
        s = float(np.sqrt(1 - LD(w) ** 2))
        k1 += [(0.0, s, w), (0.0, -s, w), (1.0e-39, s, w), (s, 0.0, w), (-s, 0.0, w)]
    k1 = np.array(k1)
    wr = rng.uniform(-0.99, 0.99, 200)
    ur, vr, wr = _unit_from_w(wr, rng.uniform(0, 2 * np.pi, 200))
    u1, v1, w1 = np.concatenate([k1[:, 0], ur]), np.concatenate([k1[:, 1], vr]), np.concatenate([k1[:, 2], wr])
    xi, yi, zi = _unit_from_w(rng.uniform(-1, 1, 20), rng.uniform(0, 2 * np.pi, 20))
    ax = np.array([(1.0, 0, 0), (0, 1.0, 0), (0, 0, 1.0), (0, 0, -1.0)])
    xi, yi, zi = np.concatenate([xi, ax[:, 0]]), np.concatenate([yi, ax[:, 1]]), np.concatenate([zi, ax[:, 2]])
    I, J = [v.ravel() for v in np.meshgrid(np.arange(xi.size), np.arange(u1.size), indexing="ij")]
    return xi[I], yi[I], zi[I], u1[J], v1[J], w1[J]


def check_rotation(probe):
    require_extended()
    ins = rotation_inputs()
    u1, w1 = ins[3], ins[5]
    assert (w1 > 0.999999999).any() and ((w1 <= 0.999999999) & (np.abs(u1) < TINY_REAL)).any() and (w1 == -1.0).any()
    got = probe("rotation", *ins)
    ref = rotation_literal(*ins)
    err = np.max([np.abs(g.astype(LD) - r).astype(np.float64) for g, r in zip(got, ref)], axis=0)
    fig = dict(n=err.size, max_err_in_eps=float(err.max() / EPS))
    print("rotation:", fig)
    assert err.max() <= 16.0 * EPS, fig
    return fig


def stokes_rotation_literal(u0, v0, w0, u1, v1, w1):
    """cos and sin of omega by the reference's route (scattering.f90:1187-1226) -- acos, + pi / 2, doubled, cos and sin --
    evaluated in float64 from the default-real costhet and rounded to default real.  Returns the two before and after the
    zeroing below 1e-6."""
    _, pj, pk = rotation_literal(u0, v0, w0, u1, v1, w1, real=np.float64)
    xnyp = np.sqrt(pk * pk + pj * pj).astype(np.float32)
    small = xnyp < np.float32(1e-10)
    with np.errstate(divide="ignore", invalid="ignore"):
        costhet = np.where(small, np.float32(1.0), (-1.0 * pj / xnyp.astype(np.float64)).astype(np.float32)).astype(np.float32)
    theta = np.arccos(costhet.astype(np.float64))
    theta = np.where(theta >= np.pi, 0.0, theta) + 0.5 * np.pi
    omega = np.where(pk < 0.0, -2.0 * theta, 2.0 * theta)
    cw, sw = np.cos(omega).astype(np.float32), np.sin(omega).astype(np.float32)
    cz = np.where(np.abs(cw) < np.float32(1e-6), np.float32(0), cw)
    sz = np.where(np.abs(sw) < np.float32(1e-6), np.float32(0), sw)
    return cw.astype(np.float64), sw.astype(np.float64), cz.astype(np.float64), sz.astype(np.float64)


@functools.lru_cache(None)
def stokes_rotation_inputs():
    """k1 general; k0 = R(k1)^T (cos T, -sin T cos t, sin T sin t): the scattering angle T with sin T >= 0.1 and the
    plane's angle t, costhet = cos t, placed >= 1e-3 rad from every multiple of pi / 4 -- so that |cos omega| = |cos 2t| and
    |sin omega| = |sin 2t| are >= 2e-3 (costhet is a default real: next to +-1 it resolves t to 3e-4 only), far outside [0.5e-6, 2e-6] where the zeroing at 1e-6 would hang on the last bit."""
    rng = np.random.default_rng(20240507)
    u1, v1, w1 = _unit_from_w(rng.uniform(-0.99, 0.99, 40), rng.uniform(0, 2 * np.pi, 40))
    T = np.array([0.1, 0.7, 1.5, 2.4, 3.0])
    t = (np.arange(8)[:, None] * (np.pi / 4) + rng.uniform(1e-3, np.pi / 4 - 1e-3, (8, 6))).ravel()
    t = np.concatenate([t, np.arange(8) * (np.pi / 4) + 1e-3, np.arange(1, 9) * (np.pi / 4) - 1e-3])
    K, TT, tt = [v.ravel() for v in np.meshgrid(np.arange(40), T, t, indexing="ij")]
    u1, v1, w1 = u1[K], v1[K], w1[K]
    p = np.array([np.cos(TT), -np.sin(TT) * np.cos(tt), np.sin(TT) * np.sin(tt)])
    h = np.sqrt(u1 * u1 + v1 * v1)
    cost, sint, sing = u1 / h, v1 / h, np.sqrt(1 - w1 * w1)
    # rows of R: (sing cost, sing sint, w1), (-sint, cost, 0), (-w1 cost, -w1 sint, sing)
    u0 = sing * cost * p[0] - sint * p[1] - w1 * cost * p[2]
    v0 = sing * sint * p[0] + cost * p[1] - w1 * sint * p[2]
    w0 = w1 * p[0] + sing * p[2]
    return u0, v0, w0, u1, v1, w1


STOKES_ROT_ABS = 4.0 * 2.0 ** -24


def check_stokes_rotation(probe):
    ins = stokes_rotation_inputs()
    cw, sw, cz, sz = stokes_rotation_literal(*ins)
    for v in (cw, sw):     # the inputs were placed for this: nothing is dropped
        assert not ((np.abs(v) >= 0.5e-6) & (np.abs(v) <= 2e-6)).any() and np.abs(v).min() > 1e-3
    got = probe("stokes_rotation", *ins)
    err = max(np.abs(got[0] - cz).max(), np.abs(got[1] - sz).max())
    fig = dict(n=cw.size, max_err_in_2_m24=float(err * 2.0 ** 24))
    print("stokes_rotation:", fig)
    assert err <= STOKES_ROT_ABS, fig
    # values exactly 0 and +-1, k1 = x axis (the rotation is then the identity): forward and back scattering
    # (xnyp < 1e-10: costhet = 1), v1pj = 0 with v1pk of either sign (costhet = -+0: omega = +-pi), v1pk = 0 (costhet = -+1)
    k0 = np.array([(1.0, 0, 0), (-1.0, 0, 0), (0, 0, 1.0), (0, 0, -1.0), (0, 1.0, 0), (0, -1.0, 0), (0.6, 0.0, -0.8), (0.6, 0.8, 0.0)])
    want_c = np.array([-1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, -1.0])
    exact = (k0[:, 0], k0[:, 1], k0[:, 2], np.ones(8), np.zeros(8), np.zeros(8))
    _, _, cz, sz = stokes_rotation_literal(*exact)
    assert np.array_equal(cz, want_c) and np.array_equal(sz, np.zeros(8))
    got = probe("stokes_rotation", *exact)
    assert np.array_equal(got[0], want_c) and np.array_equal(got[1], np.zeros(8)), got
    return fig


@functools.lru_cache(None)
def stokes_apply_inputs():
    """S with I in [0.1, 10] and a polarisation of at most I; cos and sin of omega as default reals (and the exact 0, +-1);
    Mueller ratios |M12|, |M34| <= 0.3, M22 in [0.5, 1], M33, M44 in [-1, 1] -- times M11, which is 1 for the first half
    and in (0.25, 1] for the second (scattering method 1); then S[0] <= tiny: S = 0, I = 1e-39, I = 0 with Q = 0.5."""
    rng = np.random.default_rng(20240508)
    n = 4000
    I = rng.uniform(0.1, 10.0, n)
    pol = rng.normal(size=(3, n))
    pol *= I * rng.uniform(0.0, 1.0, n) / np.sqrt((pol ** 2).sum(axis=0))
    om = rng.uniform(0, 2 * np.pi, n)
    cw, sw = np.cos(om).astype(np.float32).astype(np.float64), np.sin(om).astype(np.float32).astype(np.float64)
    cw[:4], sw[:4] = [1.0, -1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -1.0]
    M11 = np.where(np.arange(n) < n // 2, 1.0, rng.uniform(0.25, 1.0, n))
    M12, M34 = M11 * rng.uniform(-0.3, 0.3, n), M11 * rng.uniform(-0.3, 0.3, n)
    M22, M33, M44 = M11 * rng.uniform(0.5, 1.0, n), M11 * rng.uniform(-1, 1, n), M11 * rng.uniform(-1, 1, n)
    S = np.vstack([I, pol])
    S[:, -3:] = np.array([[0.0, 0, 0, 0], [1.0e-39, 0, 0, 0], [0.0, 0.5, 0, 0]]).T
    return S, cw, sw, M12, M22, M33, M34, M44, M11


def check_stokes_apply(probe):
    S, cw, sw, M12, M22, M33, M34, M44, M11 = stokes_apply_inputs()
    n = cw.size
    assert (M11 != 1.0).any() and (S[0] <= TINY_REAL).sum() == 3
    got = probe("stokes_apply", S[0], S[1], S[2], S[3], cw, sw, M12, M22, M33, M34, M44, M11)
    z, o = np.zeros(n), np.ones(n)
    mat = lambda rows: np.array(rows).transpose(2, 0, 1)       # [n, 4, 4]
    R1 = mat([[o, z, z, z], [z, cw, -sw, z], [z, sw, cw, z], [z, z, z, o]])
    Mm = mat([[M11, M12, z, z], [M12, M22, z, z], [z, z, M33, M34], [z, z, -M34, M44]])
    R2 = mat([[o, z, z, z], [z, cw, sw, z], [z, -sw, cw, z], [z, z, z, o]])
    out = np.einsum("nij,njk,nkl,nl->ni", R2, Mm, R1, S.T).T
    renorm = out[0] > TINY_REAL
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(renorm, out * (M11 * S[0] / out[0]), out)
    assert renorm[:-3].all() and not renorm[-3:].any()
    tol = 16.0 * EPS * np.sqrt((S ** 2).sum(axis=0))
    err = np.abs(got - out).max(axis=0)
    fig = dict(n=n, max_err_over_tol=float((err[tol > 0] / tol[tol > 0]).max()))
    print("stokes_apply:", fig)
    assert np.all(err <= tol), fig
    # I is conserved: S'[0] = M11 S[0] (a quotient and two products: 4 eps)
    assert np.all(np.abs(got[0][renorm] - (M11 * S[0])[renorm]) <= 4.0 * EPS * (M11 * S[0])[renorm])
    return fig


# ---- hg ---------------------------------------------------------------------------------------------------------------
NANG = 180


@functools.lru_cache(None)
def hg_inputs():
    """g: 2e5 default reals log-uniform in each decade of 1e-6 .. 1 - 2^-24 and of each sign, one random draw each; every
    16th of them again at the draws 0, 2^-24, 1/2 and 1 - 2^-24.  Returns g, rand (float64 images of default reals)."""
    rng = np.random.default_rng(20240509)
    top = 1.0 - 2.0 ** -24
    gs = []
    for d in range(-6, 0):
        lo, hi = 10.0 ** d, min(10.0 ** (d + 1), top)
        g = np.exp(rng.uniform(np.log(lo), np.log(hi), 200000)).astype(np.float32).astype(np.float64)
        g = g.clip(float(np.float32(lo)), top)
        gs += [g, -g]
    ends_g = np.array([float(np.float32(1.0e-6)), top])          # the two ends of the range themselves
    g = np.concatenate(gs + [ends_g, -ends_g])
    r = rng.integers(0, 1 << 24, g.size).astype(np.float64) / (1 << 24)
    sub = np.concatenate([g[::16], ends_g, -ends_g])
    ends = np.array([0.0, 2.0 ** -24, 0.5, top])
    g = np.concatenate([g, np.repeat(sub, ends.size)])
    r = np.concatenate([r, np.tile(ends, sub.size)])
    assert np.array_equal(g, g.astype(np.float32).astype(np.float64)) and np.abs(g).max() == top
    return g, r


def hg_special_inputs():
    """g = 0, +-tiny (the isotropic branch) and the next default real above tiny (either sign), at the four ends of the
    draw and 200 random draws"""
    rng = np.random.default_rng(20240510)
    nxt = float(np.nextafter(np.float32(TINY_REAL), np.float32(1.0)))
    g = np.array([0.0, TINY_REAL, -TINY_REAL, nxt, -nxt])
    r = np.concatenate([[0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24], rng.integers(0, 1 << 24, 200).astype(np.float64) / (1 << 24)])
    G, R = [v.ravel() for v in np.meshgrid(g, r, indexing="ij")]
    return G, R


def hg_formula(g, r, real):
    """the closed-form inverse CDF as the reference spells it (scattering.f90:1354-1383), |g| > tiny; returns cospsi, q, D"""
    rd = np.minimum(r, 1.0 - 1e-6).astype(real)
    g1 = g.astype(real)
    g2 = g1 * g1
    D = 1 - g1 + 2 * g1 * rd
    q = (1 - g2) / D
    return (1 + g2 - q * q) / (2 * g1), q, D


@functools.lru_cache(None)
def hg_reference():
    """cospsi in extended precision and the bound's unit eps (1 + q^2 (1 + 2 / D)) / (2 |g|), per sample"""
    require_extended()
    g, r = hg_inputs()
    c, q, D = hg_formula(g, r, LD)
    unit = (EPS * (1 + q * q * (1 + 2 / D)) / (2 * np.abs(g))).astype(np.float64)
    return c, unit


def hg_constant():
    """C of the bound C * unit: the smallest power of two at which numpy's unfused float64 evaluation of the same formula
    passes on these inputs, times four.  Returns (C, the largest error over unit that gave it)."""
    g, r = hg_inputs()
    ref, unit = hg_reference()
    c64 = hg_formula(g, r, np.float64)[0]
    worst = float((np.abs(c64.astype(LD) - ref).astype(np.float64) / unit).max())
    return 4.0 * 2.0 ** int(np.ceil(np.log2(worst))), worst


def check_hg(probe, C):
    require_extended()
    import mpmath
    g, r = hg_inputs()
    ref, unit = hg_reference()
    nang = np.full(g.size, float(NANG))
    nang[::7] = 10.0                                  # (the cap)
    it, c, raw = probe("hg", g, r, nang)
    assert np.all((c >= -1.0) & (c <= 1.0)), "cospsi must lie in [-1, 1]"
    assert np.array_equal(c, np.clip(raw, -1.0, 1.0))
    ratio = np.abs(raw.astype(LD) - ref).astype(np.float64) / unit
    out = (raw < -1.0) | (raw > 1.0)
    fig = dict(n=g.size, max_err_over_unit=float(ratio.max()), C=C, n_outside=int(out.sum()))
    if out.any():
        fig["outside_g_range"] = (float(np.abs(g[out]).min()), float(np.abs(g[out]).max()))
        fig["outside_draws"] = sorted(set(r[out].tolist()))[:4]
        fig["outside_max_excess"] = float((np.abs(raw[out]) - 1.0).max())
        fig["outside_of_draw0_neg_g_below_0_1"] = (int((out & (r == 0.0) & (g < 0) & (g > -0.1)).sum()), int(((r == 0.0) & (g < 0) & (g > -0.1)).sum()))
    print("hg:", fig)
    assert np.all(np.abs(c.astype(LD) - np.clip(ref, -1, 1)).astype(np.float64) <= C * unit), fig
    # itheta = floor(acos(c) 180 / pi) + 1 capped at nang for the routine's own c, where the reference's angle is >= 1e-9
    # degrees from an integer (a selection by the reference alone)
    ang_ref = (np.arccos(np.clip(ref, -1, 1)) * 180 / pi_ld()).astype(np.float64)
    sel = np.abs(ang_ref - np.rint(ang_ref)) >= 1e-9
    want = np.minimum(np.floor(np.arccos(c) * 180.0 / np.pi) + 1.0, nang)
    assert sel.mean() > 0.9 and np.array_equal(it[sel], want[sel])   # (the ends of the draw give 0 and 180 degrees)
    assert np.all((it >= 1) & (it <= nang))
    # the ends of g: the isotropic branch is 2 rand_dp - 1 exactly; just above tiny the quotient rounds to 1 and every draw
    # gives g / 2 ~ 0 where the formula's value is 2 rand - 1 -- inside the bound, which is ~1e22 there (mpmath: 60 digits)
    gs, rs = hg_special_inputs()
    its, cs, raws = probe("hg", gs, rs, np.full(gs.size, float(NANG)))
    iso = np.abs(gs) <= TINY_REAL
    assert np.array_equal(cs[iso], 2.0 * np.minimum(rs[iso], 1.0 - 1e-6) - 1.0) and np.array_equal(cs, raws)
    mpmath.mp.dps = 60
    for gi, ri, ci in zip(gs[~iso], rs[~iso], cs[~iso]):
        gm, rm = mpmath.mpf(float(gi)), mpmath.mpf(min(float(ri), 1.0 - 1e-6))
        D = 1 - gm + 2 * gm * rm
        q = (1 - gm * gm) / D
        cm = (1 + gm * gm - q * q) / (2 * gm)
        assert abs(mpmath.mpf(float(ci)) - cm) <= C * EPS * (1 + q * q * (1 + 2 / D)) / (2 * abs(gm))
        assert abs(ci) <= 1.0
    assert np.array_equal(its, np.minimum(np.floor(np.arccos(cs) * 180.0 / np.pi) + 1.0, NANG))
    # the clamped cosine gives cdapres a finite direction
    k1 = probe("cdapres_pi", np.concatenate([c, cs]), 0.3, 0.36, 0.48, 0.8)
    assert np.isfinite(k1).all()
    return fig
