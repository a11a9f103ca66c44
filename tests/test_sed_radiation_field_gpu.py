"""The mean radiation field of the SED step on the device, through the C-ABI: option "radiation_field_sed",
mcgpu_fetch_radiation_field_sed / mcgpu_reset_radiation_field_sed, mcgpu_compute_J, mcgpu_compute_UV_field, the pipeline's
``radiation_field=True`` and the refusals.  The identity that pins xJ_abs to the oracle, the models and the tolerance are
those of tests/test_sed_radiation_field_emulated.py (rtol = 1e-6, atol = 1e-8 x the largest value, no cell exempt; the
oracle's sums for two observers are the same numbers in the same order: measured difference 0).  Two orders of the same
FP64 atomic sums agree at rtol = 1e-12 (tests/test_gpu_parity.py, the MultiEngine comparison)."""
import ctypes as C

import numpy as np
import pytest

from helpers import xI_close
from mcfost_amd.host import model as M
from test_sed_radiation_field_emulated import assert_field, emu, emu_xj, field_model, oracle_xJ  # noqa: F401 (emu: a fixture)

pytestmark = pytest.mark.gpu
N_STREAMS = 64
_models = {}


def model(name):
    if name not in _models:
        _models[name] = field_model(name)
    return _models[name]


def engine(m, bits=1, where=0):
    from mcfost_amd.engine import Engine
    e = Engine(m, 1e5)
    if bits:
        e.set_option("radiation_field_sed", bits)
    if where:
        e.set_option("xj_where", where)
    return e


def oracle(m):
    from oracle import Oracle
    return Oracle(m, 1e5)


@pytest.mark.parametrize("name,lam,n2", [("2d", 4, 12), ("3d", 4, 8), ("sph", 4, 8), ("voronoi", 9, 8), ("dark", 4, 8)])
def test_device_xJ_is_the_oracles_sum_over_the_sub_bins(name, lam, n2):
    m = model(name)
    b = oracle(m).run_mono(lam, n2, seed=20 + lam, n_chunks=N_STREAMS, rt1=True, n_threads=8)
    ref = oracle_xJ(b)
    flat = name in ("2d", "sph", "dark")       # 2D grids: both homes of the row; elsewhere HBM is the only one
    rows = {}
    for where in ((1, 2) if flat else (0,)):
        e = engine(m, where=where)
        a = e.run_mono(lam, n2, seed=20 + lam, n_chunks=N_STREAMS)
        assert e.get_info("xj_lds") == (1.0 if where == 2 else 0.0)
        assert np.array_equal(a["n_sent_chunk"], b["n_sent_chunk"])
        for k, v in b["counters"].items():
            if name == "sph" and k == "crossings":   # (the midplane cone's double root: a zero-length crossing more or less,
                assert abs(a["counters"][k] - v) <= 3 + 3e-4 * v        # test_gpu_parity.test_sed_mode_on_spherical_grids)
            else:
                assert a["counters"][k] == v, k
        xJ = e.fetch_radiation_field_sed()[0]
        assert not xJ[np.arange(m.n_lambda) != lam - 1].any()
        print(name, "xj_where", where)
        assert_field(xJ[lam - 1], ref)
        rows[where] = xJ[lam - 1]
        e.close()
    if flat:
        assert np.allclose(rows[1], rows[2], rtol=1e-12, atol=0)
    else:   # the LDS row is refused where it is not built
        from mcfost_amd.engine import McgpuError
        e = engine(m, where=2)
        with pytest.raises(McgpuError, match="xj_where") as ei:
            e.run_mono(lam, n2, seed=1, n_chunks=N_STREAMS)
        assert "(4)" in str(ei.value)
        e.close()


def test_device_xJ_through_the_speculative_commit():
    """counts large enough for the speculative commit (most of every stream is deposited right after a short probe): the
    row is still the oracle's, and the plain two-pass path gives the same"""
    m, lam = model("2d"), 9
    b = oracle(m).run_mono(lam, 700, seed=49, n_chunks=16, rt1=True, n_threads=8)
    rows = []
    for spec in (1, 0):
        e = engine(m)
        e.set_option("speculation", spec)
        a = e.run_mono(lam, 700, seed=49, n_chunks=16)
        assert np.array_equal(a["n_sent_chunk"], b["n_sent_chunk"]) and a["counters"] == b["counters"]
        rows.append(e.fetch_radiation_field_sed()[0][lam - 1])
        assert_field(rows[-1], oracle_xJ(b))
        e.close()
    assert np.allclose(rows[0], rows[1], rtol=1e-12, atol=0)


def test_device_xJ_method2_and_without_ray_tracing():
    m, lam, n2 = model("2d"), 4, 10
    b = oracle(m).run_mono(lam, n2, seed=31, n_chunks=N_STREAMS, rt2=(15, 15), n_threads=8)
    ref = oracle_xJ(b, rt2=True)
    rows = {}
    for where in (1, 2):
        e = engine(m, where=where)
        a = e.run_mono(lam, n2, seed=31, n_chunks=N_STREAMS, rt2=(15, 15))
        assert np.array_equal(a["n_sent_chunk"], b["n_sent_chunk"]) and a["counters"] == b["counters"]
        rows[where] = e.fetch_radiation_field_sed()[0][lam - 1]
        assert_field(rows[where], ref)
        # a run without ray-tracing deposits still has its radiation field (the same packets)
        e.reset_radiation_field_sed()
        c = e.run_mono(lam, n2, seed=31, n_chunks=N_STREAMS, rt1=False)
        assert c["counters"] == a["counters"]
        assert e.get_info("xj_lds") == (1.0 if where == 2 else 0.0)
        assert np.allclose(e.fetch_radiation_field_sed()[0][lam - 1], rows[where], rtol=1e-12, atol=0)
        e.close()
    assert np.allclose(rows[1], rows[2], rtol=1e-12, atol=0)


def test_the_option_leaves_everything_else_alone():
    """n_sent_chunk, counters and the packet counts of the SED are those of the run without the option, xI_scatt agrees
    to the order of its atomic sums -- FP64 records, default-real records, and default-real records with the record log
    asked for ("xi_log" = 3), where the launch falls back to the atomic commit kernels.  (Default-real xI_scatt summed in
    another order: the tolerance of test_sed_mode_default_real_records for those records, rtol 1e-4 / atol 1e-5 of the
    largest value.)"""
    m, lam, n2 = model("2d"), 4, 12
    xJ64 = None
    for prec, xi_log in ((8, None), (4, 0), (4, 3)):
        res = {}
        for bits in (0, 1):
            e = engine(m, bits=bits)
            e.set_rt1()
            e.set_xI_precision(prec)
            if xi_log is not None:
                e.set_option("xi_log", xi_log)
            res[bits] = e.run_mono(lam, n2, seed=5, n_chunks=N_STREAMS)
            if xi_log == 3:   # the record log ran without the option, the atomic commit kernels with it
                assert (e.get_info("xi_rec_chunks") > 0) == (bits == 0)
            if bits:
                xJ = e.fetch_radiation_field_sed()[0][lam - 1]
                if xJ64 is None:
                    xJ64 = xJ
                assert xJ.max() > 0 and np.allclose(xJ, xJ64, rtol=1e-12, atol=0)
            e.close()
        a, b = res[0], res[1]
        assert np.array_equal(a["n_sent_chunk"], b["n_sent_chunk"]) and a["counters"] == b["counters"]
        assert np.array_equal(a["sed"][4], b["sed"][4]) and np.array_equal(a["n_sent"], b["n_sent"])
        if prec == 8:
            assert np.allclose(a["xI_scatt"], b["xI_scatt"], rtol=1e-12, atol=0)
        else:
            xI_close(b["xI_scatt"], a["xI_scatt"], rtol=1e-4, n_midplane_cells=m.cfg.n_rad, atol_rel=1e-5)


def test_rows_accumulate_per_wavelength_and_a_new_grid_drops_them():
    from mcfost_amd.engine import McgpuError
    m = model("2d")
    e = engine(m, bits=3)
    e.run_mono(4, 8, seed=1, n_chunks=N_STREAMS)
    J1, N1 = e.fetch_radiation_field_sed(xN=True)
    assert J1[3].max() > 0 and not J1[np.arange(m.n_lambda) != 3].any() and not N1[np.arange(m.n_lambda) != 3].any()
    e.run_mono(9, 8, seed=2, n_chunks=N_STREAMS)           # another wavelength: its own row, the other's untouched
    J2, N2 = e.fetch_radiation_field_sed(xN=True)
    assert np.array_equal(J2[3], J1[3]) and np.array_equal(N2[3], N1[3]) and J2[8].max() > 0
    assert not J2[[l for l in range(m.n_lambda) if l not in (3, 8)]].any()
    e.run_mono(4, 8, seed=3, n_chunks=N_STREAMS)           # the same wavelength with another seed adds
    J3, N3 = e.fetch_radiation_field_sed(xN=True)
    assert np.array_equal(J3[8], J2[8]) and np.array_equal(N3[8], N2[8])
    e.reset_radiation_field_sed()
    Jz, Nz = e.fetch_radiation_field_sed(xN=True)
    assert not Jz.any() and not Nz.any()
    e.run_mono(4, 8, seed=3, n_chunks=N_STREAMS)           # ... what that second run deposits by itself
    Jb, Nb = e.fetch_radiation_field_sed(xN=True)
    assert np.allclose(J3[3], J1[3] + Jb[3], rtol=1e-12, atol=0) and np.array_equal(N3[3], N1[3] + Nb[3])
    assert (Jb[3] > 0).any()
    # xN_abs: positive exactly where xJ_abs is
    assert np.array_equal(Nb > 0, Jb > 0)
    e._upload(m, 1e5)                                       # a new grid drops the arrays
    with pytest.raises(McgpuError, match="radiation_field_sed") as ei:
        e.fetch_radiation_field_sed()
    assert "(5)" in str(ei.value)                           # MCGPU_ERR_STATE
    e.run_mono(4, 8, seed=3, n_chunks=N_STREAMS)           # the next run allocates them again, zeroed
    Jc, Nc = e.fetch_radiation_field_sed(xN=True)
    assert np.allclose(Jc, Jb, rtol=1e-12, atol=0) and np.array_equal(Nc, Nb)
    e.close()
    # without the option nothing is kept
    e = engine(m, bits=0)
    e.run_mono(4, 8, seed=3, n_chunks=N_STREAMS)
    with pytest.raises(McgpuError, match="radiation_field_sed") as ei:
        e.fetch_radiation_field_sed()
    assert "(5)" in str(ei.value)
    e.close()


@pytest.mark.parametrize("name,lam", [("2d", 4), ("voronoi", 9)])
def test_xN_is_the_emulated_lanes_count(emu, name, lam):  # noqa: F811
    """integers, the same packets: array_equal"""
    m = model(name)
    e = engine(m, bits=3)
    a = e.run_mono(lam, 8, seed=11, n_chunks=N_STREAMS)
    xJ, xN = e.fetch_radiation_field_sed(xN=True)
    e.close()
    c = emu_xj(emu, oracle(m), lam, 8, 11, n_chunks=N_STREAMS)
    assert list(a["counters"].values()) == c["counters"]
    assert np.array_equal(xN[lam - 1], c["xN"].astype(np.float64))
    assert np.array_equal(xN > 0, xJ > 0)
    assert 0 < xN.sum() <= a["counters"]["crossings"]


# ---- compute_J / compute_UV_field against a float64 restatement of output.f90:2280-2286 and :2458-2519 ----------------
HP, C_LIGHT = 6.626070040e-34, 299792458.0


def span_f32(xmin, xmax, n):
    """utils.f90:43-62: a running sum in default real"""
    f = np.float32
    out = np.zeros(n, f)
    dx = f((f(xmax) - f(xmin)) / f(n - 1))
    out[0] = f(xmin)
    for i in range(1, n):
        out[i] = f(out[i - 1] + dx)
    return out


def interp_ref(y, x, xp):
    """utils.f90:190 ff.: no extrapolation; the search `do j = 2, n-1` (x increasing)"""
    n = len(x)
    if xp < x.min():
        return y[0]
    if xp > x.max():
        return y[n - 1]
    j = 2
    while j <= n - 1 and not x[j - 1] > xp:
        j += 1
    frac = (xp - x[j - 2]) / (x[j - 1] - x[j - 2])
    return y[j - 2] * (1.0 - frac) + y[j - 1] * frac


def J_ref(xJ, J0, n_sent, E_stars, E_disk, tab_lambda, volume):
    pe = HP * C_LIGHT ** 2 / 2.0 * (E_stars + E_disk) / n_sent * tab_lambda * float(np.float32(1.0e-6))
    return (xJ + J0) * pe[:, None] / volume[None, :]


def UV_ref(xJ, J0, n_sent, E_stars, E_disk, tab_lambda, volume):
    pe = HP * C_LIGHT ** 2 / 2.0 * (E_stars + E_disk) / n_sent
    J = (xJ + J0) * pe[:, None] / volume[None, :]
    lamb = tab_lambda * float(np.float32(1e-6))
    wl = (span_f32(0.0912, 0.2, 200) * np.float32(1e-6)).astype(np.float64)
    delta_wl = (wl[-1] - wl[0]) / float(np.float32(200) - np.float32(1.0))
    G = np.zeros(J.shape[1])
    for ic in range(J.shape[1]):
        Ji = np.array([interp_ref(J[:, ic], lamb, w) for w in wl])
        G[ic] = (Ji.sum() - 0.5 * (Ji[0] + Ji[-1])) * delta_wl / float(np.float32(2.67e-6))
    return G


def _abi(e, fn, n_sent, E_stars, E_disk, tab_lambda, J0, out):
    d = C.POINTER(C.c_double)
    arrs = [np.ascontiguousarray(x, np.float64) for x in (n_sent, E_stars, E_disk, tab_lambda)]
    j0 = np.ascontiguousarray(J0, np.float64) if J0 is not None else None
    return fn(e.ctx, *[a.ctypes.data_as(d) for a in arrs], j0.ctypes.data_as(d) if j0 is not None else None,
              out.ctypes.data_as(C.POINTER(C.c_float)))


def test_compute_J_and_UV_field_against_the_restatement():
    m = model("2d")
    e = engine(m)
    for lam, seed in ((2, 1), (4, 2), (9, 3)):
        e.run_mono(lam, 8, seed=seed, n_chunks=N_STREAMS, rt1=False)
    xJ = e.fetch_radiation_field_sed()[0]
    assert (xJ.max(axis=1) > 0).sum() == 3
    nl, nc = m.n_lambda, m.n_cells
    rng = np.random.default_rng(7)
    n_sent = rng.integers(500, 5000, nl).astype(np.float64)
    E_stars, E_disk = np.asarray(m.E_stars, np.float64), rng.uniform(0.1, 1.0, nl) * np.asarray(m.E_stars, np.float64).max()
    vol = np.asarray(m.grid["volume"], np.float64)[:nc]
    J0 = rng.uniform(0.0, 1.0, (nl, nc)) * xJ.max()
    grids = {"the model's": np.asarray(m.lam, np.float64),
             "covers the band": np.geomspace(0.05, 3000.0, nl),
             "starts above the band": np.geomspace(0.3, 3000.0, nl),
             "ends inside the band": np.geomspace(0.01, 0.15, nl)}
    for gname, tab in grids.items():
        for j0 in (None, J0):
            z = np.zeros_like(xJ) if j0 is None else j0
            Jio, G = np.zeros((nl, nc), np.float32), np.zeros(nc, np.float32)
            assert _abi(e, e.lib.mcgpu_compute_J, n_sent, E_stars, E_disk, tab, j0, Jio) == 0
            assert _abi(e, e.lib.mcgpu_compute_UV_field, n_sent, E_stars, E_disk, tab, j0, G) == 0
            Jr, Gr = J_ref(xJ, z, n_sent, E_stars, E_disk, tab, vol), UV_ref(xJ, z, n_sent, E_stars, E_disk, tab, vol)
            print(gname, "J0" if j0 is not None else "no J0", "max rel J %.2e G %.2e" %
                  (np.abs(Jio / np.where(Jr != 0, Jr, 1) - 1)[Jr != 0].max(), np.abs(G / np.where(Gr != 0, Gr, 1) - 1)[Gr != 0].max() if (Gr != 0).any() else 0.0))
            assert np.allclose(Jio, Jr, rtol=1e-6, atol=0) and np.allclose(G, Gr, rtol=1e-6, atol=0)
            assert (Jr > 0).any() and (j0 is None or (Gr > 0).all())
    # the engine's own wrappers are these calls with the model's tables
    assert np.allclose(e.compute_J(n_sent, E_disk, J0), J_ref(xJ, J0, n_sent, E_stars, E_disk, grids["the model's"], vol), rtol=1e-6, atol=0)
    assert np.allclose(e.compute_UV_field(n_sent, E_disk), UV_ref(xJ, 0 * xJ, n_sent, E_stars, E_disk, grids["the model's"], vol), rtol=1e-6, atol=0)
    # a wavelength without packets: the reference divides by zero
    ns0 = n_sent.copy()
    ns0[6] = 0.0
    for fn, out in ((e.lib.mcgpu_compute_J, np.zeros((nl, nc), np.float32)), (e.lib.mcgpu_compute_UV_field, np.zeros(nc, np.float32))):
        assert _abi(e, fn, ns0, E_stars, E_disk, grids["the model's"], None, out) == 3      # MCGPU_ERR_ARG
        assert "wavelength 7" in e.lib.mcgpu_last_error(e.ctx).decode()
    e.close()


def test_pipeline_returns_J_and_UV_field():
    from mcfost_amd.host import pipeline as P
    m = M.build_model(M.small(lsepar_pola=False))
    e = engine(m, bits=0)
    lambdas = [3, 9]
    plain = P.temperature_and_sed(P.EngineBackend(e), m, 20000, 8, lambdas=lambdas, seed=3, n_chunks=16)
    assert set(plain) == {"Tdust", "sed_mc", "n_sent", "sed_rt", "sed_rt_stars", "seconds", "thermal_counters", "E_disk",
                          "sed_crossings"}
    out = P.temperature_and_sed(P.EngineBackend(e), m, 20000, 8, lambdas=lambdas, seed=3, n_chunks=16, radiation_field=True)
    assert set(out) == set(plain) | {"J", "UV_field"}
    # (two temperature steps on the device differ in the order of their sums, so the two SED steps are not compared)
    ns = np.where(out["n_sent"] > 0, out["n_sent"], 1.0)
    J, G = e.compute_J(ns, m.extra["E_disk"]), e.compute_UV_field(ns, m.extra["E_disk"])
    assert np.array_equal(out["J"], J) and np.array_equal(out["UV_field"], G)
    assert out["J"].shape == (m.n_lambda, m.n_cells) and out["J"].dtype == np.float32 and out["UV_field"].shape == (m.n_cells,)
    rows = np.zeros(m.n_lambda, bool)
    rows[[l - 1 for l in lambdas]] = True
    assert (out["J"][rows].max(axis=1) > 0).all() and not out["J"][~rows].any()
    e.close()


def test_the_multi_context_calls_refuse_by_name():
    from mcfost_amd.engine import McgpuError, MultiEngine
    m = model("2d")

    def refused(what, call):
        with pytest.raises(McgpuError, match=what) as ei:
            call()
        assert "(4)" in str(ei.value), str(ei.value)          # MCGPU_ERR_UNSUPPORTED

    me = MultiEngine(m, 1e5, devices=(0,))
    me.engines[0].set_option("radiation_field_sed", 1)
    refused("mcgpu_multi_run_mono: option radiation_field_sed", lambda: me.run_mono(4, 8, seed=1, n_chunks=8))
    refused("mcgpu_multi_run_sed: option radiation_field_sed", lambda: me.run_sed([4], 8, m.extra["Tdust"], n_chunks=8))
    me.engines[0].set_option("radiation_field_sed", 0)
    me.run_mono(4, 8, seed=1, n_chunks=8)                     # (switched off again the calls run)
    me.close()
