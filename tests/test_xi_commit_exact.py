"""The SED commit pass's ATOMIC deposit staging on the GPU, compared bit for bit (mcgpu_probe_xi_commit).

wave_deposit_records (FP64 records), deposit_rt1_wave_f32 (the packed default-real layout, with the flight's weights and
with dust classes), deposit_rt1_wave_row (the default of BASELINE config 2), the placement of the per-lane results they
read (rt1_store_weights / row_put) and angles_scatt_rt1_wave exist only for whole waves: the one-lane emulation never runs
them, and the end-to-end comparisons with the oracle (rtol 1e-6 .. 1e-4 on sums over psup, a few outliers allowed) would
not notice a deposit lost once in ten thousand crossings, a value in the neighbouring observer's or the other origin's
place, a stale row, or a write into a sub-bin's padding.

Here the library's own functions run on deposits the test chooses (tests/xi_commit_cases.py): path lengths in [1, 7],
weights and Stokes values in [-7, 7] with zeros, Mueller columns and ratios small integers, cosw / sinw in {-1, 0, 1}.
Every product and partial sum is an integer below 2^24 (default real) or 2^53 (FP64) -- every case asserts that on its
reference --, so the sums are the same in any order and the device's array must EQUAL an int64 sum made with numpy and
placed with the Python mirrors of the layout.  There is no tolerance in the deposit tests.  The arrays (5 cells x 2 x 1 or 3
sub-bins plus 7 slack sub-bins) start from non-zero integers; slack, every padding float of a sub-bin and the unused slots
of an FP64 record must come back unchanged; with contributions the fetched I must be star + thermal exactly.

The edges of the staging arithmetic (K lanes serve a record, floor(64 / K) records per atomic instruction, TILE_UNROLL = 8
rounds of tile reads in flight; the default-real paths: 16 lanes per staged place, 4 x TILE_UNROLL = 32 places per trip):
  K = 5 (Stokes + contributions): 12 records per instruction, lanes 60-63 stage but never serve; trips at 12 / 13
  K = 4: 16 / 17;   K = 2: 32 / 33 (and the default-real paths' 32 places);   K = 1 and every path: 63 / 64
xi_commit_cases.edge_schedule visits both sides of each with every wave, next to single lanes (0, 37, 63), waves without a
deposit, rounds without a new flight, and waves that are all stellar, all thermal or mixed (split layout: lines nobody
reaches, lines only one origin reaches).

Which layout the observer counts yield is tabulated in xi_commit_cases (SPLIT_POLA, SPLIT_NOPOLA) and asserted from
xi32_layout in test_layouts_of_the_observer_counts."""
import numpy as np
import pytest

import xi_commit_cases as K
from mcfost_amd.engine import xi32_layout, xi32_offset
from mcfost_amd.host import model as M

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2, 3)      # deposit_rt1_wave (FP64) | deposit_rt1_wave_f32 | deposit_rt1_wave_row | deposit_rt1_wave_f32, dust classes
COMBOS = [(nRT, pola, contrib) for nRT in K.NRT_ALL for pola in (False, True) for contrib in (False, True)]
N_CLASSES, N_LAMBDA, P_LAMBDA = 3, 2, 2


@pytest.fixture(scope="module")
def eng():
    """one small engine: the probe uses its context (device, stream) and none of its tables"""
    from mcfost_amd.engine import Engine
    e = Engine(M.build_model(M.small()), 1000)
    yield e
    e.close()


def deposit(eng, rng, path, sch, nRT, pola, contrib, grid, threads, x0=None):
    """run `sch` through `path` and check everything every case owes; returns the array after the deposits"""
    f32 = path != 0
    if x0 is None:
        x0 = K.start_array(rng, f32, nRT, pola, contrib, sch.n_az)
    n = sch.R * sch.T
    kw = {}
    if path in (1, 2):
        w = K.weights_of(rng, sch, nRT, pola)
        vals = K.values_from_weights(sch, w)
        kw["weights"] = w.reshape(n, nRT, -1)
        mu = np.full((6, K.NANG + 1), 99.0, np.float32)          # (never read)
    else:
        it, cw, sw, S = K.angles_of(rng, sch, nRT, 7 if path == 0 else 3)
        kw.update(itheta=it.reshape(n, nRT), cosw=cw.reshape(n, nRT), sinw=sw.reshape(n, nRT), S=S.reshape(n, 4))
        if path == 0:
            mu = K.mueller(rng)
            vals = K.values_from_angles(sch, it, cw, sw, S, mu, pola)
        else:      # the class tables in HBM, the column of p_lambda; the LDS columns must not be read
            mu = np.full((6, K.NANG + 1), 99.0, np.float32)
            vtab = K.mueller(rng, N_CLASSES, N_LAMBDA)
            cls = rng.integers(0, N_CLASSES, K.N_CELLS).astype(np.int32)
            vals = K.values_from_angles(sch, it, cw, sw, S, vtab, pola, cls, P_LAMBDA)
            kw.update(vtab=vtab, cell_class=cls, p_lambda=P_LAMBDA)
    want = K.reference(sch, vals, x0, f32, nRT, pola, contrib)
    raw, fetched = eng.probe_xi_commit(path, sch.where.reshape(n, 4), sch.l.reshape(n), x0, nRT, pola, contrib, grid, threads,
                                       K.N_CELLS, K.N_THETA, sch.n_az, mu, **kw)
    assert raw.dtype == want.dtype and raw.shape == want.shape
    bad = np.argwhere(raw != want)
    assert bad.size == 0, (path, nRT, pola, contrib, grid, threads, len(bad), bad[:8].tolist(),
                           [(float(raw[tuple(b)]), float(want[tuple(b)]), float(x0[tuple(b)])) for b in bad[:8]])
    ns = K.n_sub(sch.n_az)
    assert np.array_equal(raw[ns:], x0[ns:])                                    # the slack sub-bins
    pad = ~K.mapped_places(f32, nRT, pola, contrib)
    assert np.array_equal(raw[..., pad], x0[..., pad])                          # padding floats / unused slots of a record
    if f32:
        assert np.array_equal(fetched, K.fetched_reference(want, nRT, pola, contrib, sch.n_az))
        if contrib:
            nS = 4 if pola else 1
            assert np.array_equal(fetched[:, :, 0], fetched[:, :, nS + 1] + fetched[:, :, nS + 3])
    assert (want != x0).any()
    return raw


def test_layouts_of_the_observer_counts():
    for nRT in K.NRT_ALL:
        assert xi32_layout(nRT, True, True)["split"] == K.SPLIT_POLA[nRT], nRT
        assert xi32_layout(nRT, False, True)["split"] == K.SPLIT_NOPOLA[nRT], nRT
        assert not xi32_layout(nRT, True, False)["split"] and not xi32_layout(nRT, False, False)["split"]
    # an observer straddles a line (interleaved, 5 values from q * 5 on); a stellar origin shares a line with Stokes values (split)
    assert xi32_offset(5, True, True, 3, 1) == 15 and xi32_offset(5, True, True, 3, 2) == 16
    assert xi32_offset(10, True, True, 0, 5) == 30 and xi32_offset(10, True, True, 9, 3) == 29
    # no Stokes tracking, split: nA = 0, the stellar origins from 0, the thermal ones from the next line on
    assert xi32_offset(10, False, True, 0, 2) == 0 and xi32_offset(10, False, True, 0, 4) == 16


@pytest.mark.parametrize("nRT,pola,contrib", COMBOS)
@pytest.mark.parametrize("path", PATHS)
def test_edges_every_layout(eng, path, nRT, pola, contrib):
    """the edge schedule (25 rounds, one workgroup of as many waves as fit, up to 8) for every observer count, with and
    without Stokes tracking and contributions"""
    rng = np.random.default_rng([11, path, nRT, pola, contrib])
    threads = K.threads_that_fit(path, nRT, pola, contrib)
    n_az = 3 if nRT % 2 else 1
    deposit(eng, rng, path, K.edge_schedule(rng, threads, n_az), nRT, pola, contrib, 1, threads)


@pytest.mark.parametrize("pola,contrib", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("path", PATHS)
def test_all_lanes_one_subbin(eng, path, pola, contrib):
    """all 64 lanes of all 8 waves of a 512-thread workgroup deposit into ONE sub-bin, three rounds running, all stellar /
    all thermal / mixed by wave; then the same from three workgroups"""
    rng = np.random.default_rng([12, path, pola, contrib])
    for grid in (1, 3):
        T = 512 * grid
        sch = K.Schedule(rng, np.ones((3, T), bool), np.zeros((3, T), bool), 3, star_by_wave=True, one_bin=(2, 1, 3))
        deposit(eng, rng, path, sch, 3, pola, contrib, grid, 512)


@pytest.mark.parametrize("lanes", [[0], [37], [63], [60, 61, 62, 63], list(range(12)), list(range(13))])
@pytest.mark.parametrize("path", PATHS)
def test_few_lanes_of_one_wave(eng, path, lanes):
    """one wave, the same few lanes deposit in each of four rounds (ten observers, Stokes tracking, contributions: K = 5,
    the split layout); new flights only in rounds 0 and 2"""
    rng = np.random.default_rng([13, path] + lanes)
    on = np.zeros((4, 64), bool)
    on[:, lanes] = True
    fresh = np.zeros((4, 64), bool)
    fresh[2] = True
    deposit(eng, rng, path, K.Schedule(rng, on, fresh, 1), 10, True, True, 1, 64)


@pytest.mark.parametrize("threads,grid", [(64, 1), (64, 3), (256, 1), (256, 3), (512, 1), (512, 3)])
@pytest.mark.parametrize("nRT,pola,contrib", [(10, True, True), (5, True, True), (11, False, True), (6, True, False)])
@pytest.mark.parametrize("path", PATHS)
def test_random_schedules_and_launch_geometry(eng, path, nRT, pola, contrib, threads, grid):
    """32 rounds, 40 % of the lanes deposit, 30 % start a flight; workgroups of 64, 256 and 512 threads, grids of 1 and 3
    (the rows' stride blockDim.x, the per-wave tile offset)"""
    rng = np.random.default_rng([14, path, nRT, pola, contrib, threads, grid])
    sch = K.random_schedule(rng, threads * grid, 3)
    deposit(eng, rng, path, sch, nRT, pola, contrib, grid, threads)


@pytest.mark.parametrize("path", PATHS)
def test_rows_survive_the_neighbours_rewrites(eng, path):
    """every lane deposits in every round; in each round after the first only every third lane starts a new flight (a
    different third each time): the others' results must be those of their own last flight"""
    rng = np.random.default_rng([15, path])
    R, T = 9, 256
    fresh = (np.arange(T)[None, :] + np.arange(R)[:, None]) % 3 == 0
    deposit(eng, rng, path, K.Schedule(rng, np.ones((R, T), bool), fresh, 3), 10, True, True, 1, T)


@pytest.mark.parametrize("path", PATHS)
def test_a_wave_without_deposits_between_waves_with(eng, path):
    """per round every other wave has no deposit at all (the early return), alternating"""
    rng = np.random.default_rng([16, path])
    R, T = 6, 512
    on = ((np.arange(T) // 64)[None, :] + np.arange(R)[:, None]) % 2 == 0
    deposit(eng, rng, path, K.Schedule(rng, on, rng.random((R, T)) < 0.5, 1, star_by_wave=True), 8, True, True, 1, T)


@pytest.mark.parametrize("path", PATHS)
def test_two_launches_accumulate(eng, path):
    rng = np.random.default_rng([17, path])
    mid = deposit(eng, rng, path, K.random_schedule(rng, 256, 3, R=8), 4, True, True, 1, 256)
    deposit(eng, rng, path, K.random_schedule(rng, 256, 3, R=8), 4, True, True, 1, 256, x0=mid)


def test_refusals(eng):
    """more LDS than 160 KB, a deposit beyond the array, a scattering-angle bin beyond the tables: MCGPU_ERR_ARG"""
    from mcfost_amd.engine import McgpuError
    rng = np.random.default_rng(18)
    assert K.lds_bytes(0, 16, 512, True, True) > 160 * 1024 >= K.lds_bytes(0, 16, 256, True, True)
    sch = K.random_schedule(rng, 512, 1, R=2)
    n = sch.R * sch.T
    it, cw, sw, S = K.angles_of(rng, sch, 16, 7)
    args = dict(itheta=it.reshape(n, 16), cosw=cw.reshape(n, 16), sinw=sw.reshape(n, 16), S=S.reshape(n, 4))
    x0 = K.start_array(rng, False, 16, True, True, 1)
    with pytest.raises(McgpuError):
        eng.probe_xi_commit(0, sch.where.reshape(n, 4), sch.l.reshape(n), x0, 16, True, True, 1, 512, K.N_CELLS, K.N_THETA, 1,
                            K.mueller(rng), **args)
    sch = K.random_schedule(rng, 64, 1, R=2)
    n = sch.R * sch.T
    w = K.weights_of(rng, sch, 2, False).reshape(n, 2, 1)
    x0 = K.start_array(rng, True, 2, False, False, 1)
    for col, v in ((0, K.N_CELLS + 1), (1, K.N_THETA + 1), (2, 2)):
        where = sch.where.reshape(n, 4).copy()
        where[5, :3] = (1, 1, 1)
        where[5, col] = v
        with pytest.raises(McgpuError):
            eng.probe_xi_commit(1, where, sch.l.reshape(n), x0, 2, False, False, 1, 64, K.N_CELLS, K.N_THETA, 1, K.mueller(rng), weights=w)
    it, cw, sw, S = K.angles_of(rng, sch, 2, 7)
    it[0, 3, 1] = K.NANG + 1
    x0 = K.start_array(rng, False, 2, False, False, 1)
    with pytest.raises(McgpuError):
        eng.probe_xi_commit(0, sch.where.reshape(n, 4), sch.l.reshape(n), x0, 2, False, False, 1, 64, K.N_CELLS, K.N_THETA, 1,
                            K.mueller(rng), itheta=it.reshape(n, 2), S=S.reshape(n, 4))


# ---- angles_scatt_rt1_wave ----------------------------------------------------------------------------------------------
A_NANG, A_THREADS, A_ROUNDS = 180, 256, 5
NEED = (0, 1, 7, 33, 64)        # lanes of a wave that start a flight in a round: wave w, round r -> NEED[(w + r) % 5]


def angle_case(nRT, seed):
    rng = np.random.default_rng([19, nRT, seed])
    n_incl = 5 if nRT == 10 else nRT                 # (ten observers: five inclinations x two azimuths, q = ibin + n_incl iaz)
    incl = np.arccos(rng.uniform(0.05, 0.95, n_incl))
    az = rng.uniform(0, 2 * np.pi, nRT // n_incl)
    rt_w = np.cos(incl)
    q = np.arange(nRT)
    rt_u, rt_v = np.sin(incl[q % n_incl]) * np.cos(az[q // n_incl]), np.sin(incl[q % n_incl]) * np.sin(az[q // n_incl])
    T, R = A_THREADS, A_ROUNDS
    d = rng.normal(size=(R, T, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    need = np.zeros((R, T), bool)
    for r in range(R):
        need[r] = K.lanes_mask(rng, T, lambda w: NEED[(w + r) % 5])
    star = rng.random((R, T)) < 0.5
    return dict(rng=rng, nRT=nRT, rt_u=rt_u, rt_v=rt_v, rt_w=rt_w, dirs=d, need=need, star=star, T=T, R=R)


def run_angles(eng, c, S, mu, pola, by_wave, with_mu, row, contrib=False):
    n = c["R"] * c["T"]
    out = eng.probe_rt1_angles(c["dirs"].reshape(n, 3), S.reshape(n, 4), c["need"].reshape(n), c["star"].reshape(n), c["rt_u"], c["rt_v"],
                               c["rt_w"], mu, pola, 1, c["T"], by_wave, with_mu=with_mu, row=row, contrib=contrib)
    return {k: v.reshape((c["R"], c["T"]) + v.shape[1:]) for k, v in out.items()}


def angles_reference(c):
    """angles_scatt_rt1 (dust_ray_tracing.f90:409-476) with rotation (utils.f90) in float64 numpy for every (round, lane,
    observer); `ok`: the pairs whose result does not hinge on the last bits -- acos nang / pi at least 1e-2 of a bin from a
    bin edge, |cos omega| and |sin omega| outside [5e-7, 2e-6]: conditions on this reference alone"""
    u, v, w = (c["dirs"][..., k][..., None] for k in range(3))
    ur, vr = c["rt_u"], c["rt_v"]
    wr = c["rt_w"][np.arange(c["nRT"]) % c["rt_w"].size]
    cs = (ur * u + vr * v + wr * w).astype(np.float32).astype(np.float64)       # cos_scatt is a default real
    quot = np.arccos(np.clip(cs, -1, 1)) * A_NANG / np.pi
    k = np.clip(np.floor(quot + 0.5), 1, A_NANG).astype(np.int32)                # nint, clamped to 1..nang
    ok = (np.abs(quot + 0.5 - np.round(quot + 0.5)) >= 1e-2) & (np.abs(cs) < 1)
    u1, v1, w1 = -ur, -vr, -wr                                                   # rotation(u, v, w, -u_obs, -v_obs, -w_obs)
    theta = np.arctan2(v1, u1)
    cost, sint, sing = np.cos(theta), np.sin(theta), np.sqrt(1.0 - w1 * w1)
    assert (w1 <= 0.999999999).all() and (np.abs(u1) > 1e-30).all()              # (the generic branch of rotation)
    prod = cost * u + sint * v
    v1pj = cost * v - sint * u
    v1pk = sing * w - w1 * prod
    xnyp = np.sqrt(v1pk * v1pk + v1pj * v1pj)
    costhet = np.where(xnyp < 1e-10, 1.0, -v1pj / np.where(xnyp < 1e-10, 1.0, xnyp))
    th = np.arccos(np.clip(costhet, -1, 1))
    th = np.where(th >= np.pi, 0.0, th) + np.pi / 2
    omega = np.where(v1pk < 0.0, -2.0 * th, 2.0 * th)
    cosw, sinw = np.cos(omega), np.sin(omega)
    for x in (cosw, sinw):
        ok &= (np.abs(x) < 5e-7) | (np.abs(x) > 2e-6)
    cosw = np.where(np.abs(cosw) < 1e-6, 0.0, cosw)
    sinw = np.where(np.abs(sinw) < 1e-6, 0.0, sinw)
    return k, cosw, sinw, ok


def weights_reference(k, cosw, sinw, S, mu):
    """the flight's four deposit weights in float64: the Mueller elements are default-real products (angles_scatt_rt1_one),
    everything after them double"""
    f = np.float32
    s11 = mu[0][k]
    s12, s22, s33 = f(-s11 * mu[1][k]), f(s11 * mu[2][k]), f(-s11 * mu[3][k])
    s34, s44 = f(-s11 * mu[4][k]), f(-s11 * mu[5][k])
    s11, s12, s22, s33, s34, s44 = (x.astype(np.float64) for x in (s11, s12, s22, s33, s34, s44))
    S0, S1, S2, S3 = (S[..., j][..., None] for j in range(4))
    C2 = cosw * S1 - sinw * S2
    C3 = sinw * S1 + cosw * S2
    D1, D2 = s11 * S0 + s12 * C2, s12 * S0 + s22 * C2
    D3, D4 = s33 * C3 - s34 * S3, s34 * C3 + s44 * S3
    return np.stack((D1, -cosw * D2 - sinw * D3, -sinw * D2 + cosw * D3, D4), axis=-1)


def carried(c, x):
    """per (round, lane): the results of the lane's last flight (zero before its first)"""
    r = np.maximum.accumulate(np.where(c["need"], np.arange(c["R"])[:, None], -1), axis=0)
    y = np.take_along_axis(x, np.broadcast_to(np.maximum(r, 0).reshape(r.shape + (1,) * (x.ndim - 2)), x.shape), axis=0)
    return y, r >= 0


def row_place(nRT, pola, contrib, q, t):
    """where a flight's row holds weight t of observer q (t = 0 with contributions: the place of the stellar origin, which
    in the split arrangement stands for both origins)"""
    nS = 4 if pola else 1
    if contrib and t == 0:
        return xi32_offset(nRT, pola, contrib, q, nS + 1)
    return xi32_offset(nRT, pola, contrib, q, t)


@pytest.mark.parametrize("nRT", [1, 3, 10, 11])
def test_angles_by_wave_equal_by_lane(eng, nRT):
    """angles_scatt_rt1_wave and the per-lane angles_scatt_rt1 leave the same bytes: need masks of 0, 1, 7, 33 and 64 lanes
    (items = lanes x nRT cross multiples of 64), angles and weights, slots and rows; a lane without `need` keeps what it had"""
    c = angle_case(nRT, 0)
    rng = c["rng"]
    S = rng.integers(-7, 8, (c["R"], c["T"], 4)).astype(np.float64)
    mu = rng.integers(1, 8, (6, A_NANG + 1)).astype(np.float32)
    keep = ~c["need"][1:]
    for pola, with_mu, row, contrib in [(False, False, False, False), (True, False, False, False), (False, True, False, False),
                                        (True, True, False, False), (False, True, True, False), (True, True, True, False),
                                        (False, True, True, True), (True, True, True, True)]:
        a = run_angles(eng, c, S, mu, pola, True, with_mu, row, contrib)
        b = run_angles(eng, c, S, mu, pola, False, with_mu, row, contrib)
        assert sorted(a) == sorted(b)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), (nRT, pola, with_mu, row, contrib, key)
            assert np.array_equal(a[key][1:][keep].view(np.uint8), a[key][:-1][keep].view(np.uint8)), key
            assert a[key].view(np.uint8).any()


@pytest.mark.parametrize("nRT", [1, 3, 10, 11])
def test_angles_against_the_reference_restated(eng, nRT):
    c = angle_case(nRT, 1)
    rng = c["rng"]
    k, cosw, sinw, ok = angles_reference(c)
    assert ok.mean() >= 0.9                                   # (of the (direction, observer) draws)
    (k_c, cw_c, sw_c, ok_c), had = zip(*(carried(c, x) for x in (k, cosw, sinw, ok)))
    had = had[0]
    ok_c = ok_c & had[..., None]
    assert ok_c.sum() > 0.5 * ok_c.size
    # the scattering-angle bins (Stokes tracking on and off: the same function)
    Sint = rng.integers(-7, 8, (c["R"], c["T"], 4)).astype(np.float64)
    mu_int = rng.integers(1, 8, (6, A_NANG + 1)).astype(np.float32)
    for pola in (False, True):
        got = run_angles(eng, c, Sint, mu_int, pola, True, False, False)
        assert np.array_equal(got["itheta"][ok_c], k_c[ok_c])
        assert (got["itheta"][~had] == 0).all()
    # without Stokes tracking, integer mu and S: the weight is Stokes(1) x s11(k), exactly; as a slot and as a row
    S_c = carried(c, Sint)[0]
    want = (S_c[..., :1] * mu_int[0][k_c]).astype(np.float32)
    got = run_angles(eng, c, Sint, mu_int, False, True, True, False)["itheta"].view(np.float32)
    assert np.array_equal(got[ok_c], want[ok_c])
    got = run_angles(eng, c, Sint, mu_int, False, True, True, True)["row"]
    places = [row_place(nRT, False, False, q, 0) for q in range(nRT)]
    assert np.array_equal(got[..., places][ok_c], want[ok_c])
    # with Stokes tracking: within one unit in the last place of default real of the reference's value, plus 1e-12 of the
    # row's largest weight (both sides evaluate the same double expression and round once)
    S = rng.uniform(-1, 1, (c["R"], c["T"], 4))
    mu = rng.uniform(0.1, 1.0, (6, A_NANG + 1)).astype(np.float32)
    mu[1:] *= rng.choice([-1.0, 1.0], (5, A_NANG + 1)).astype(np.float32)
    w64 = weights_reference(k_c, cw_c, sw_c, carried(c, S)[0], mu)           # [R, T, nRT, 4]
    w32 = w64.astype(np.float32)
    tol = np.spacing(np.abs(w32)).astype(np.float64) + 1e-12 * np.abs(w64).max(axis=(2, 3), keepdims=True)
    slots = run_angles(eng, c, S, mu, True, True, True, False)
    got = np.concatenate((slots["cosw"].view(np.float32).reshape(w32.shape[:3] + (2,)),
                          slots["sinw"].view(np.float32).reshape(w32.shape[:3] + (2,))), axis=-1)
    err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    print("slots: largest error / tolerance", (err / tol)[ok_c].max())
    assert (err <= tol)[ok_c].all()
    for contrib in (False, True):
        row = run_angles(eng, c, S, mu, True, True, True, True, contrib)["row"]
        lay = xi32_layout(nRT, True, contrib)
        star = carried(c, c["star"])[0]
        for q in range(nRT):
            for t in range(4):
                g = row[..., row_place(nRT, True, contrib, q, t)].astype(np.float64)
                okq = ok_c[..., q]
                if contrib and t == 0 and not lay["split"]:    # interleaved: the flux in the place of its origin, 0 in the other
                    o_th = xi32_offset(nRT, True, True, q, 7)
                    g_th = row[..., o_th].astype(np.float64)
                    assert (g[okq & ~star] == 0).all() and (g_th[okq & star] == 0).all()
                    g = np.where(star, g, g_th)
                assert (np.abs(g - w32[..., q, t]) <= tol[..., q, t])[okq].all(), (contrib, q, t)
