"""Grains in radiative equilibrium out of LTE (lRE_nLTE), the GPU suite, through the C-ABI: the probe of one re-emission
event, the tables built on the device, frozen and live launches, Temp_finale_nLTE, the lRE_nLTE term of
repartition_energie and the refusals.  Yardstick: tests/nlte_restatement.py (numpy, from the reference's lines)."""
import dataclasses

import numpy as np
import pytest

from helpers import rel_rms
from mcfost_amd.host import model as M
from nlte_cases import N_TOTAL, compare_events, nlte_model, random_events, smooth_field
from nlte_restatement import repartition_nlte_term, temp_finale_nlte

pytestmark = pytest.mark.gpu


def _engine(m, nl, n_tot=N_TOTAL, J0=True, **kw):
    from mcfost_amd.engine import Engine
    e = Engine(m, n_tot)
    e.set_nlte(nl, **kw)
    if J0:
        e.set_J0(nl["J0"])
    return e


def _vol(m):
    return np.ascontiguousarray(np.asarray(m.grid["volume"], np.float64)[:m.n_cells])


def test_probe_against_the_restatement():
    m, nl = nlte_model()
    nl["J0"] = smooth_field(m, nl)
    e = _engine(m, nl)
    n = 100000
    icell, lambda0, r1, r2 = random_events(m, nl, n)
    got = e.probe_reemission_nlte(icell, lambda0, r1, r2)
    info = compare_events(got, nl, m.tab_Temp, _vol(m), m.L_packet_th(N_TOTAL), icell, lambda0, r1, r2)
    assert set(info["grains"]) == set(range(2, nl["n_grains"] + 1)) and info["T_span"] == (2, m.tab_Temp.size)
    e.close()


def test_tables_built_on_the_device():
    """mcgpu_init_reemission_nlte = model.init_nlte with the reference's default-real literal, to the tolerances
    tests/test_init_reemission.py holds the LTE tables to (exp / log differ from libm in the last place)"""
    from mcfost_amd.engine import McgpuError
    m, nl = nlte_model(real_literal=True)
    e = _engine(m, nl, build_on_device=True)
    with pytest.raises(McgpuError, match="mcgpu_init_reemission_nlte"):
        e.run_thermal(100, seed=1)
    lE, cdf = e.init_reemission_nlte()
    assert np.allclose(lE, nl["log_E_em_1grain"], rtol=0, atol=1e-12)
    assert np.allclose(cdf, nl["kdB_dT_1grain_nLTE_CDF"], rtol=0, atol=1e-13)
    # ... and the events run on them
    nl2 = dict(nl, log_E_em_1grain=lE, kdB_dT_1grain_nLTE_CDF=cdf, J0=smooth_field(m, nl))
    e.set_J0(nl2["J0"])
    icell, lambda0, r1, r2 = random_events(m, nl, 20000, seed=5)
    compare_events(e.probe_reemission_nlte(icell, lambda0, r1, r2), nl2, m.tab_Temp, _vol(m), m.L_packet_th(N_TOTAL),
                   icell, lambda0, r1, r2)
    # a table that decreases with T is refused
    bad = dict(nl, log_E_em_1grain=nl["log_E_em_1grain"][::-1].copy())
    with pytest.raises(McgpuError, match="increase with T"):
        e.set_nlte(bad)
    e.close()


@pytest.mark.parametrize("grid", ["cyl2d", "cyl3d"])
@pytest.mark.parametrize("mix", ["only_nlte", "mixed"])
def test_frozen_launch(grid, mix):
    cfg = M.small(n_rad=12, nz=6, n_az=8, l3D=True) if grid == "cyl3d" else M.small()
    m, nl = nlte_model(cfg, nlte_range=(1, 16) if mix == "only_nlte" else (1, 6))
    assert (nl["Proba_abs_RE_LTE"] is None) == (mix == "only_nlte")
    n = 20000
    e = _engine(m, nl, n_tot=n)
    e.set_option("nlte_stats", 1)
    prior = np.asarray(m.grid["volume"], np.float64)[:m.n_cells] * 1e-3 + 1.0
    runs = []
    for _ in range(2):
        # (non-LTE grains alone: a frozen launch reads J0 and needs no E_prior)
        r = e.run_thermal(n, seed=5, frozen=True, E_prior=prior if mix == "mixed" else None)
        _, xJ = e.fetch_radiation_field(xN=False)
        runs.append((r, xJ))
    (a, xJa), (b, xJb) = runs
    c = a["counters"]
    assert a["n_sent"].sum() == n
    assert c["escaped"] + c["killed_star"] == n and c["packets"] == n
    assert c["absorptions"] > n // 10 and e.get_info("nlte_events") > 0
    if mix == "only_nlte":
        assert e.get_info("nlte_events") == c["absorptions"]
    else:
        assert 0 < e.get_info("nlte_events") < c["absorptions"]
    # the absorbed energy of the (LTE) opacity the context holds: E_abs = sum_lambda kappa_abs_LTE * xJ_abs
    assert xJa.shape == (m.n_lambda, m.n_cells)
    assert np.allclose((np.asarray(m.kappa_abs_LTE)[:, None] * xJa).sum(axis=0), a["E_abs"], rtol=1e-10)
    # two runs with the same seed
    assert np.array_equal(a["n_sent"], b["n_sent"]) and a["counters"] == b["counters"]
    assert np.array_equal(a["sed"][4], b["sed"][4])
    assert np.allclose(xJa, xJb, rtol=1e-9, atol=0.0)
    # Temp_finale_nLTE on the fetched xJ_abs, and from the device's own
    L = m.L_packet_th(n)
    want = temp_finale_nlte(nl, m.tab_Temp, _vol(m), L, float(m.tab_Temp[0]), xJb)
    got = e.temp_finale_nlte(xJb)
    assert got.shape == (m.n_cells, nl["n_grains"]) and (want > 2.0 * m.tab_Temp[0]).any()
    assert np.allclose(got, want, rtol=2e-6, atol=0.0)
    assert np.allclose(e.temp_finale_nlte(), want, rtol=2e-6, atol=0.0)
    # switched off again: the launch is the LTE launch it was
    e.set_nlte(None)
    from mcfost_amd.engine import Engine
    e0 = Engine(m, n)
    x, y = e.run_thermal(n, seed=5, frozen=True, E_prior=prior), e0.run_thermal(n, seed=5, frozen=True, E_prior=prior)
    assert x["counters"] == y["counters"] and np.allclose(x["E_abs"], y["E_abs"], rtol=1e-9)
    e.close()
    e0.close()


def _one_grain(m):
    ka32 = np.asarray(m.kappa_abs_LTE, np.float64).astype(np.float32)
    grains = dict(n_grains=1, C_abs=np.ones((m.n_lambda, 1), np.float32), n_grains_k=np.ones(1))
    return M.init_nlte(m, grains, np.ones(1), (1, 1), C_abs_norm=ka32[:, None])


def _pooled(pairs):
    """rel. rms over the cells, pooled over pairs of runs (the rms of one pair is a noisy estimate: below)"""
    return float(np.sqrt(np.mean([rel_rms(a, b, 0.0) ** 2 for a, b in pairs])))


def test_live_launch_one_grain_is_the_lte_temperature():
    """All dust in ONE non-LTE grain whose cross section is kappa_abs_LTE: Tdust_1grain(1, :) is the LTE temperature.
    Yardstick: the LTE path on the same model and packet count -- the relative rms between two LTE runs with different
    seeds over the cells both resolve; the non-LTE run against an LTE run may exceed it by at most 1.5x (two independent
    samples of one quantity have the same spread; the half covers the per-grain table's missing tab_Temp(1) floor).

    Both figures are estimated from several runs: the rms of ONE pair of 4e5-packet runs over 200 cells is itself noisy (a few
    cells with rare long paths carry much of it) -- measured between LTE runs alone 5.1e-3, 5.8e-3 and 8.8e-3 for three
    pairs --, and a bound of 1.5x on the ratio of two such single figures fails by chance (1.30x / 1.36x / 1.56x in three
    runs of the single-pair form).  Eight LTE runs (28 pairs) and eight non-LTE runs (64 pairs against the LTE runs), pooled
    as root mean square, estimate the same two quantities (measured: 1.19x / 1.16x / 1.17x in three runs of this test).  The two Temp_finale formulas agree to 3e-7 on one accumulator
    (checked below), and the frozen comparison (next test) shows the transport unbiased; what is left between live runs of
    different kernels is their in-flight temperature estimate: the existing single-role LTE kernel differs from the role
    schedule's by +6e-3 in the mean of the cold cells, the non-LTE kernel by -2e-3."""
    from mcfost_amd.engine import Engine
    m = M.build_model(M.small())
    nl = _one_grain(m)
    n = 400000
    e0 = Engine(m, n)
    lte = [e0.temp_finale(e0.run_thermal(n, seed=s)["E_abs"]) for s in range(11, 19)]
    e = _engine(m, nl, n_tot=n)
    non = []
    for s in range(21, 29):
        r = e.run_thermal(n, seed=s)
        assert r["counters"]["escaped"] + r["counters"]["killed_star"] == n
        non.append(e.temp_finale_nlte()[:, 0])
    # one accumulator through both formulas: the per-grain table without floor against log_Qcool
    _, xJ = e.fetch_radiation_field(xN=False)
    floor = 3.0 * float(m.tab_Temp[0])
    both = np.all(np.array(lte + non) > floor, axis=0)
    assert both.sum() > 0.5 * m.n_cells
    assert np.allclose(e.temp_finale_nlte(xJ)[both, 0], e0.temp_finale((np.asarray(m.kappa_abs_LTE)[:, None] * xJ).sum(axis=0))[both], rtol=1e-5)
    lte_vs_lte = _pooled([(lte[i][both], lte[j][both]) for i in range(len(lte)) for j in range(i)])
    nlte_vs_lte = _pooled([(a[both], b[both]) for a in non for b in lte])
    msg = "rel. rms of Tdust over %d cells: LTE vs LTE %.4e, non-LTE (one grain) vs LTE %.4e (%.2fx)" % (
        both.sum(), lte_vs_lte, nlte_vs_lte, nlte_vs_lte / lte_vs_lte)
    print(msg)
    assert nlte_vs_lte <= 1.5 * lte_vs_lte, msg
    e.close()
    e0.close()


def test_frozen_one_grain_transport_is_the_lte_transport():
    """The same degenerate case with the temperatures held fixed: E_prior for the LTE launch, J0 = the xJ_abs of the same
    earlier run for the non-LTE one, so every re-emission draws from the same temperature in both (formulas equal to
    3e-7).  What is left between the two is sampling noise: the absorbed energy of the non-LTE launches against the LTE
    launches' is within 1.5x of LTE against LTE (three seeds each, pooled) -- no bias in the non-LTE kernel's transport,
    deposits or accumulator layout."""
    from mcfost_amd.engine import Engine
    m = M.build_model(M.small())
    nl = _one_grain(m)
    n = 1000000
    e0 = Engine(m, n)
    e0.set_option("radiation_field", 2)
    E0 = e0.run_thermal(n, seed=3)["E_abs"]
    _, xJ0 = e0.fetch_radiation_field(xN=False)
    e0.set_option("radiation_field", 0)
    lte = [e0.temp_finale(e0.run_thermal(n, seed=s, frozen=True, E_prior=E0)["E_abs"]) for s in (31, 32, 33)]
    e = _engine(m, nl, n_tot=n, J0=False)
    e.set_J0(xJ0 + nl["J0"])
    non = [e0.temp_finale(e.run_thermal(n, seed=s, frozen=True)["E_abs"]) for s in (41, 42, 43)]
    both = np.all(np.array(lte + non) > 3.0 * float(m.tab_Temp[0]), axis=0)
    lte_vs_lte = _pooled([(lte[i][both], lte[j][both]) for i in range(3) for j in range(i)])
    nlte_vs_lte = _pooled([(a[both], b[both]) for a in non for b in lte])
    offset = float(np.mean([(a[both] / b[both] - 1.0).mean() for a in non for b in lte]))
    msg = "frozen, rel. rms over %d cells: LTE vs LTE %.4e, non-LTE vs LTE %.4e, mean offset %+.2e" % (both.sum(), lte_vs_lte, nlte_vs_lte, offset)
    print(msg)
    assert nlte_vs_lte <= 1.5 * lte_vs_lte, msg
    e.close()
    e0.close()


def _thin_disk(tau_midplane=5e-3):
    """small() with its dust mass scaled until the radial optical depth of the midplane at the most opaque wavelength is
    tau_midplane; returns the model and, per cell, G = integral over the cell of dV / (4 pi d^2): the path length a packet
    of an unattenuated point source at the origin leaves in the cell, on average"""
    m = M.build_model(M.small())
    g, nc = m.grid, m.n_cells
    n_rad, nz = int(g["n_rad"]), int(g["nz"])
    ci = np.asarray(g["cell_map_i"], np.int64)[:nc]
    cj = np.abs(np.asarray(g["cell_map_j"], np.int64)[:nc])
    r_lim = np.asarray(g["r_lim"], np.float64)
    kf = np.asarray(m.kappa_factor, np.float64)
    mid = cj == 1
    tau = float(np.sum(np.asarray(m.kappa, np.float64).max() * kf[:nc][mid] * (r_lim[ci[mid]] - r_lim[ci[mid] - 1])))
    m = dataclasses.replace(m, kappa_factor=kf * (tau_midplane / tau))
    dz = np.asarray(g["z_lim"], np.float64)[n_rad + ci - 1]          # z_lim(ri, 2): the column's cell height
    sub = (np.arange(32) + 0.5) / 32
    r = r_lim[ci - 1][:, None] + (r_lim[ci] - r_lim[ci - 1])[:, None] * sub[None, :]        # [nc, 32]
    z = ((cj - 1) * dz)[:, None] + dz[:, None] * sub[None, :]
    w = r[:, :, None] * np.ones_like(z)[:, None, :]
    mean = (w / (4.0 * np.pi * (r[:, :, None] ** 2 + z[:, None, :] ** 2))).sum(axis=(1, 2)) / w.sum(axis=(1, 2))
    return m, np.asarray(g["volume"], np.float64)[:nc] * mean


def test_live_launch_thin_disk_known_answer_per_grain():
    """A disk thin at every wavelength (midplane optical depth 5e-3), 16 grain sizes, all non-LTE: per cell and grain the
    temperature that solves sum C_abs_norm B(T) = sum C_abs_norm J_star for the diluted stellar field, computed in numpy on
    the same tables (J_star(icell, lambda) = packets emitted at lambda x the mean path of an unattenuated packet in the
    cell).  Yardstick: the same thin disk through the LTE path against ITS analytic value; the per-grain temperatures get
    3x that deviation as their bound, and the smallest grain is hotter than the largest in every resolved cell."""
    from mcfost_amd.engine import Engine
    m, G = _thin_disk()
    n = 2000000
    P = np.diff(np.asarray(m.spectre_emission_cumul, np.float64))
    J_star = n * P[:, None] * G[None, :]                              # [n_lambda, n_cells]
    e0 = Engine(m, n)
    r0 = e0.run_thermal(n, seed=5)
    assert r0["counters"]["absorptions"] + r0["counters"]["scatterings"] < 0.05 * n          # thin
    T_lte = e0.temp_finale(r0["E_abs"])
    T_lte_an = e0.temp_finale((np.asarray(m.kappa_abs_LTE, np.float64)[:, None] * J_star).sum(axis=0))
    floor = 3.0 * float(m.tab_Temp[0])
    sel = (T_lte_an > floor) & (T_lte > floor)
    assert sel.sum() > 0.9 * m.n_cells
    dev_lte = rel_rms(T_lte[sel], T_lte_an[sel], 0.0)
    grains = M.synthetic_grains(m, 16)
    _, dens = M.settled_grain_density(m, grains, xi=0.0, per_cell=False, n_classes=1)
    nl = M.init_nlte(m, grains, dens, (1, 16))
    e = _engine(m, nl, n_tot=n)
    e.run_thermal(n, seed=6)
    T1 = e.temp_finale_nlte()
    T1_an = temp_finale_nlte(nl, m.tab_Temp, _vol(m), m.L_packet_th(n), float(m.tab_Temp[0]), J_star)
    dev = np.array([rel_rms(T1[sel, k], T1_an[sel, k], 0.0) for k in range(16)])
    msg = "thin disk, rel. rms over %d cells against the analytic temperature: LTE %.3e; grains %s" % (
        sel.sum(), dev_lte, " ".join("%.3e" % d for d in dev))
    print(msg)
    print("T of the smallest / largest grain: %.1f / %.1f K (innermost cell), %.1f / %.1f K (outermost)" % (
        T1[sel, 0].max(), T1[sel, -1].max(), T1[sel, 0].min(), T1[sel, -1].min()))
    assert dev_lte < 0.05, msg                     # (the yardstick itself measures the analytic field, not a mistake in it)
    assert np.all(dev <= 3.0 * dev_lte), msg
    assert np.all(T1[sel, 0] > T1[sel, -1])
    e.close()
    e0.close()


def test_repartition_energie_with_the_non_lte_term():
    """after mcgpu_set_Tdust_1grain the cells' emission holds the lRE_nLTE term (thermal_emission.f90:1832-1850); without the
    call the results are bit for bit what they are (tolerances of tests/test_repartition_energie.py: 1e-12 / 1e-14)"""
    m, nl = nlte_model(nlte_range=(1, 6))
    e = _engine(m, nl)
    rng = np.random.default_rng(2)
    Tdust = (20.0 * np.exp(rng.normal(0.0, 0.8, m.n_cells))).astype(np.float32)
    T1 = (30.0 * np.exp(rng.normal(0.0, 0.8, (m.n_cells, nl["n_grains"])))).astype(np.float32)
    T1[::5, 2] = 0.0
    for lam in (m.n_lambda // 2, m.n_lambda - 4, m.n_lambda):      # (wavelengths these temperatures emit at)
        base = e.repartition_energie(lam, Tdust)
        e.set_Tdust_1grain(T1)
        got = e.repartition_energie(lam, Tdust)
        term = repartition_nlte_term(nl, float(m.lam[lam - 1]), lam, T1, _vol(m), m.l_dark_zone)
        p0 = np.asarray(base["prob_E_cell"])
        want_E = base["E_disk"] + term.sum()
        assert term.sum() > 0.0 and np.isclose(got["E_disk"], want_E, rtol=1e-12)
        # prob_E_cell is the running sum of E_cell over its total: with the term, that of E_cell + term
        want_p = (p0 * base["E_disk"] + np.concatenate([[0.0], np.cumsum(term)])) / want_E
        assert np.allclose(np.asarray(got["prob_E_cell"]), want_p, rtol=1e-12, atol=1e-14)
        e.set_Tdust_1grain(None)
        again = e.repartition_energie(lam, Tdust)
        assert again["E_disk"] == base["E_disk"] and np.array_equal(np.asarray(again["prob_E_cell"]), p0)
        # the grains' temperatures belong to the non-LTE tables: switching those off (or replacing them) drops the term
        e.set_Tdust_1grain(T1)
        e.set_nlte(None)
        off = e.repartition_energie(lam, Tdust)
        assert off["E_disk"] == base["E_disk"] and np.array_equal(np.asarray(off["prob_E_cell"]), p0)
        e.set_nlte(nl)
        fewer = dict(nl, n_grains=3, C_abs_norm=nl["C_abs_norm"][:, :3].copy(), kabs_nLTE_CDF=nl["kabs_nLTE_CDF"][:, :4].copy(),
                     grain_density=nl["grain_density"][:, :3].copy(), log_E_em_1grain=nl["log_E_em_1grain"][:, :3].copy(),
                     kdB_dT_1grain_nLTE_CDF=nl["kdB_dT_1grain_nLTE_CDF"][:, :3].copy())
        e.set_Tdust_1grain(T1)
        e.set_nlte(fewer)
        assert e.repartition_energie(lam, Tdust)["E_disk"] == base["E_disk"]
        e.set_nlte(nl)
    e.close()


def test_out_of_scope_is_refused_by_name():
    from mcfost_amd.engine import Engine, McgpuError, MultiEngine
    m, nl = nlte_model()

    def refused(what, call):
        with pytest.raises(McgpuError, match=what) as ei:
            call()
        assert "(4)" in str(ei.value), str(ei.value)          # MCGPU_ERR_UNSUPPORTED

    def launch_refused(model, tables, what):
        e = Engine(model, 1000)
        e.set_nlte(tables)
        refused(what, lambda: e.run_thermal(1000, seed=1))
        e.close()

    e = Engine(m, 1000)
    refused("lnRE", lambda: e.set_nlte(nl, n_grains_nRE=3))
    e.run_thermal(1000, seed=1)                               # (the refused call left the context an LTE one)
    e.close()
    mv = M.build_model(M.small())
    M.init_variable_dust(mv)
    launch_refused(mv, nl, "variable dust")
    mw = M.build_model(M.small())
    M.init_mrw(mw)
    launch_refused(mw, nl, "random walk")
    from test_scattering_method1 import _model as method1_model      # (method 1 runs on a variable-dust context)
    m1, g, _, dens = method1_model()
    M.init_scattering_method1(m1, g, dens)
    launch_refused(m1, M.init_nlte(m1, M.synthetic_grains(m1, 16), np.ones(16), (1, 16)), "scattering method 1")
    ms, nls = nlte_model(M.small(grid_type=2))
    launch_refused(ms, nls, "spherical grid")
    mvo = M.build_voronoi_model(M.small(), 1500, seed=2)
    launch_refused(mvo, M.init_nlte(mvo, M.synthetic_grains(mvo, 16), np.ones(16), (1, 16)), "Voronoi grid")
    me = MultiEngine(m, 1000, devices=(0,))
    me.engines[0].set_nlte(nl)
    refused("mcgpu_multi_run_thermal with non-LTE grains", lambda: me.run_thermal(1000, seed=1))
    me.close()


@pytest.mark.parametrize("nlte_range", [(1, 6), (1, 16)])
def test_pipeline_hands_the_grain_temperatures_to_the_sed_step(nlte_range):
    """host/pipeline.py: the temperature step returns Tdust_1grain when the engine holds non-LTE grains, and the SED step's
    emission tables hold their term; the ray-traced SED (no per-grain emissivity in the ray tracer) is refused"""
    from mcfost_amd.host import pipeline as P
    m, nl = nlte_model(M.small(RT_n_incl=3), nlte_range=nlte_range)
    n, lam = 100000, m.n_lambda - 4
    e = _engine(m, nl, n_tot=n)
    with pytest.raises(NotImplementedError, match="per-grain"):
        P.temperature_and_sed(P.EngineBackend(e), m, n, 200, lambdas=[lam], seed=3, n_chunks=8)
    with pytest.raises(Exception, match="no non-LTE launch"):          # (refused before anything ran)
        e.temp_finale_nlte()
    g = P.temperature_and_sed(P.EngineBackend(e), m, n, 200, lambdas=[lam], seed=3, n_chunks=8, ray_tracing=False)
    T1 = g["Tdust_1grain"]
    assert T1.shape == (m.n_cells, nl["n_grains"]) and T1.max() > 100.0
    assert np.array_equal(T1, e.temp_finale_nlte())
    term = repartition_nlte_term(nl, float(m.lam[lam - 1]), lam, T1, _vol(m), m.l_dark_zone).sum()
    e.set_Tdust_1grain(None)
    base = e.repartition_energie(lam, g["Tdust"])["E_disk"]
    if nlte_range == (1, 16):      # no LTE grain: the SED step's emission is the grains' alone, not counted twice
        assert np.all(g["Tdust"] == 0.0) and base == 0.0
    else:
        assert base > 0.0
    assert term > 0.0 and np.isclose(g["E_disk"][lam], base + term, rtol=1e-12)
    assert g["n_sent"][lam - 1] > 0
    e.close()
