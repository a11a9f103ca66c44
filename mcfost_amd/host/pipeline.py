"""Host-side sequence of a "temperature + SED" run (BASELINE config 2) over the engine: what
``transfert_poussiere`` does around the packet loops (dust_transfer.f90:188-433) --

    run_thermal_mc      (:575-688)   one temperature iteration + Temp_finale
    repartition_energie (thermal_emission.f90:1771)   emission tables of the SED step from Tdust
    run_sed_mc          (:828-1042)  per wavelength: the monochromatic packet loop (SED bins + xI_scatt),
                                     then the ray-traced SED of the dust (dust_map, RT method 1)
    run_image_mc        (:692-824)   one wavelength: the image-mode packet loop (a fixed number of packets per stream),
                                     then per observer the source function, dust_map's pixels, the stars' discs and,
                                     if asked, the optical-depth maps (``image`` below)

The Fortran host keeps doing this itself; this mirror drives the same C-ABI calls from Python
for the tests, ``tools/run_config2.py`` and as an executable description of the call order.  ``backend`` is
anything with the Engine's methods (``EngineBackend`` below; the tests pass the CPU oracle through an adapter)."""
from __future__ import annotations

import time

import numpy as np

from . import model as M


class EngineBackend:
    """The MI355X engine (mcfost_amd.engine.Engine) behind the pipeline's four calls."""

    def __init__(self, engine):
        self.e = engine

    def run_thermal(self, n, seed):
        return self.e.run_thermal(n, seed=seed)

    def temp_finale(self, E_abs):
        return self.e.temp_finale(E_abs)

    def temp_approx_diffusion_vertical(self, Tdust, ri_in, ri_out, zj_sup):
        return self.e.temp_approx_diffusion_vertical(Tdust, ri_in, ri_out, zj_sup)[0]

    def nlte_grains(self):
        """None: LTE grains only; "only": non-LTE grains alone (lonly_nLTE); "mixed": both"""
        nl = getattr(self.e, "nlte", None)
        return None if nl is None else ("only" if nl.get("Proba_abs_RE_LTE") is None else "mixed")

    def temp_finale_nlte(self):
        """Temp_finale_nLTE after a temperature step with grains out of LTE (Engine.set_nlte): Tdust_1grain [n_cells, n_grains],
        handed on to the SED step's repartition_energie (its lRE_nLTE term); None without such grains."""
        if getattr(self.e, "nlte", None) is None:
            return None
        T1 = self.e.temp_finale_nlte()
        self.e.set_Tdust_1grain(T1)
        return T1

    def repartition_energie(self, lam, Tdust):
        """repartition_energie(lam) on the device (mcgpu_repartition_energie): the wavelength's emission tables stay in
        HBM for the run_mono that follows; returns E_disk(lam)."""
        self._tables = (lam, self.e.repartition_energie(lam, Tdust, fetch=False))
        return self._tables[1]["E_disk"]

    def run_mono(self, lam, n2, seed, n_chunks):
        t = getattr(self, "_tables", None)
        return self.e.run_mono(lam, n2, seed=seed, n_chunks=n_chunks, fetch_xI=False,
                               device_tables=t[1] if t is not None and t[0] == lam else None)

    def dust_map(self, lam, Tdust, res, E_disk):
        return self.e.dust_map_sed(lam, Tdust, res["n_sent"][lam - 1], E_disk)[0]

    def radiation_field_start(self):
        """The SED step keeps xJ_abs per cell and wavelength (option "radiation_field_sed"), from zero."""
        self.e.set_option("radiation_field_sed", 1)
        self.e.reset_radiation_field_sed()

    def radiation_field_outputs(self, n_sent, E_disk):
        """ecriture_J(2)'s J [n_lambda, n_cells] and compute_UV_field's G [n_cells] from what the wavelength loop left"""
        return self.e.compute_J(n_sent, E_disk), self.e.compute_UV_field(n_sent, E_disk)

    def stars_map(self, lam, star_flux, seed):
        return self.e.stars_map_sed(lam, star_flux, seed=seed)


    # --- run_image_mc ---
    def run_image_mc(self, lam, n_photons_image, seed, n_chunks, method):
        """mc_photon_loop with lmono0 (dust_transfer.f90:711-713): every stream sends exactly n_photons_image packets; the
        deposits of ray tracing method 1 (xI_scatt) or 2 (I_spec) stay on the device."""
        t = getattr(self, "_tables", None)
        return self.e.run_mono(lam, 10 ** 12, n_phot_lim=float(n_photons_image), seed=seed, n_chunks=n_chunks, fetch_xI=False,
                               device_tables=t[1] if t is not None and t[0] == lam else None,
                               rt2=(15, 15) if method == 2 else None)

    def dust_image(self, lam, Tdust, res, E_disk, npix_x, npix_y, map_size, zoom, ang_disque):
        return self.e.dust_map_image(lam, Tdust, res["n_sent"][lam - 1], E_disk, npix_x, npix_y, map_size, zoom=zoom,
                                     ang_disque=ang_disque)[0]

    def dust_image_method2(self, lam, ibin, Tdust, res, E_disk, npix_x, npix_y, map_size, zoom):
        ns = res["n_sent"][lam - 1]
        self.e.init_dust_source_fct2(lam, ibin, None, None, Tdust, ns, E_disk)
        return self.e.rt2_dust_map_image(lam, Tdust, ns, E_disk, npix_x, npix_y, map_size, zoom=zoom)[0]

    def stars_image(self, lam, star_flux, npix_x, npix_y, map_size, zoom, seed, ang_disque):
        return self.e.stars_map_image(lam, star_flux, npix_x, npix_y, map_size, zoom=zoom, seed=seed, ang_disque=ang_disque)[0]

    def tau_maps(self, lam, npix_x, npix_y, map_size, zoom, tau, ang_disque):
        return self.e.tau_maps(lam, npix_x, npix_y, map_size, zoom=zoom, tau=tau, ang_disque=ang_disque)[:2]

    # --- disk-structure outputs ---
    def column(self, type, lam=None, gas_density=None, abundance=None):
        """compute_column on the device: column [4, n_cells]; a ray stopped by the cap on crossings is an error here"""
        col, n_capped, _ = self.e.compute_column(type, lam=lam, gas_density=gas_density, abundance=abundance)
        if n_capped:
            raise RuntimeError("compute_column: %d rays did not leave the grid within the cap on crossings" % n_capped)
        return col

    def integ_tau(self, lam, angle):
        return self.e.integ_tau(lam, angle)

    # --- molecular lines ---
    def line_map(self, mol, **kw):
        """emission_line_map on the device: (spectrum, continu); a ray stopped by the cap on crossings is an error here"""
        spec, cont, n_capped, _ = self.e.line_map(mol, **kw)
        if n_capped:
            raise RuntimeError("line_map: %d rays did not leave the grid within the cap on crossings" % n_capped)
        return spec, cont


def temperature_and_sed(backend, m, n_thermal, n_photons_lambda, lambdas=None, seed=1, n_chunks=None,
                        ray_tracing=True, diff_approx=None, radiation_field=False):
    """Returns Tdust, the nine Monte Carlo SED arrays ``sed_mc`` (9, N_phi, N_thet, n_lambda), ``n_sent``
    (packets sent per wavelength in the SED step), ``sed_rt`` (n_lambda, nRT, N_type_flux; dust only) and the
    wall time of each stage.  ``radiation_field`` (an engine backend): the SED step also keeps its mean radiation field,
    and ``J`` (n_lambda, n_cells; default real, W m^-2: ``ecriture_J(2)``, output.f90:2280-2286; zero rows for the wavelengths
    not in ``lambdas``) and ``UV_field`` (n_cells; Habing: ``compute_UV_field``, output.f90:2458-2519, which interpolates
    over ALL wavelengths: run them all for a meaningful value) are returned too."""
    t = {}
    nlte = backend.nlte_grains() if hasattr(backend, "nlte_grains") else None
    if nlte is not None and ray_tracing:   # (said before anything runs or changes the context)
        raise NotImplementedError("ray-traced SED with grains out of LTE: the ray tracer's thermal emissivity has no per-grain "
                                  "term (dust_ray_tracing.f90:860-890); run with ray_tracing=False")
    if radiation_field and not hasattr(backend, "radiation_field_start"):
        raise NotImplementedError("radiation_field=True needs a backend that keeps the SED step's xJ_abs (EngineBackend)")
    t0 = time.perf_counter()
    th = backend.run_thermal(int(n_thermal), seed)
    Tdust = backend.temp_finale(th["E_abs"])
    # grains out of LTE (lRE_nLTE): their own temperatures, which the SED step's emission tables then hold
    Tdust_1grain = backend.temp_finale_nlte() if nlte is not None else None
    if nlte == "only":
        # no LTE grain: the reference's kappa_abs_LTE is 0 and the LTE term of repartition_energie with it; the context's
        # kappa_abs_LTE is the whole dust's here (the deposits of E_abs), so the LTE term is switched off by its temperature
        Tdust = np.zeros_like(Tdust)
    t["thermal"] = time.perf_counter() - t0
    if diff_approx is not None:  # ldiff_approx with a dark zone: dust_transfer.f90:316 / :659
        t0 = time.perf_counter()
        Tdust = backend.temp_approx_diffusion_vertical(Tdust, *diff_approx)
        t["diffusion"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    on_device = hasattr(backend, "repartition_energie")   # the engine builds each wavelength's tables itself (:924)
    if not on_device:
        M.repartition_energie(m, Tdust)
    E_disk = {} if on_device else dict(enumerate(m.extra["E_disk"], start=1))
    t["repartition_energie"] = time.perf_counter() - t0
    nl = m.n_lambda
    lambdas = list(lambdas) if lambdas is not None else list(range(1, nl + 1))
    sed = np.zeros((9, m.cfg.N_phi, m.cfg.N_thet, nl))
    n_sent = np.zeros(nl)
    rt = m.rt
    sed_rt = np.zeros((nl, rt["RT_n_incl"] * rt["RT_n_az"], rt["N_type_flux"]))
    sed_rt_stars = np.zeros((nl, rt["RT_n_incl"] * rt["RT_n_az"]))
    t["sed_mc"] = t["ray_tracing"] = 0.0
    if radiation_field:
        backend.radiation_field_start()
    sed_crossings = 0.0   # cell crossings of the SED step's committed packets, all wavelengths (each one a set of deposits)
    for lam in lambdas:
        if on_device:
            t0 = time.perf_counter()
            E_disk[lam] = backend.repartition_energie(lam, Tdust)
            t["repartition_energie"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        r = backend.run_mono(lam, int(n_photons_lambda), seed + lam, n_chunks)
        t["sed_mc"] += time.perf_counter() - t0
        sed[..., lam - 1] = r["sed"][..., lam - 1]
        n_sent[lam - 1] = r["n_sent"][lam - 1]
        sed_crossings += float(r["counters"]["crossings"]) if "counters" in r else 0.0
        if ray_tracing:
            t0 = time.perf_counter()
            sed_rt[lam - 1] = backend.dust_map(lam, Tdust, r, E_disk[lam])
            if hasattr(backend, "stars_map"):   # compute_stars_map (dust_transfer.f90:1583-1586): added to type 1 by the caller
                sed_rt_stars[lam - 1] = backend.stars_map(lam, stars_flux_factor(m, lam), seed + 7919 * lam)
            t["ray_tracing"] += time.perf_counter() - t0
    if on_device:   # what sed_flux() and the callers' ray-tracing calls read
        Ed = np.zeros(nl)
        for lam, v in E_disk.items():
            Ed[lam - 1] = v
        m.extra["E_disk"] = Ed
    out = dict(Tdust=Tdust, sed_mc=sed, n_sent=n_sent, sed_rt=sed_rt, sed_rt_stars=sed_rt_stars, seconds=t,
               thermal_counters=th["counters"], E_disk=E_disk, sed_crossings=sed_crossings)
    if Tdust_1grain is not None:
        out["Tdust_1grain"] = Tdust_1grain
    if radiation_field:
        # (a wavelength that was not run has a zero row of xJ_abs and no packets: any count but 0 gives its zero row of J)
        ran = np.zeros(nl, bool)
        ran[[lam - 1 for lam in lambdas]] = True
        out["J"], out["UV_field"] = backend.radiation_field_outputs(np.where(ran, n_sent, 1.0), np.asarray(m.extra["E_disk"], float))
    return out


def stars_flux_factor(m, lam):
    """``factor * prob_E_star(lambda, :)`` of compute_stars_map (dust_transfer.f90:1657-1659, :1819): the flux an
    unobscured star sends to the observer, in the units of Stokes_ray_tracing."""
    pc_to_AU, AU_to_Rsun = 648000.0 / np.pi, 149597870700.0 / 6.957e8
    factor = float(m.E_stars[lam - 1]) * float(m.lam[lam - 1]) * 1.0e-6 / (m.cfg.distance * pc_to_AU * AU_to_Rsun) ** 2 * 1.35e-12
    cdf = np.asarray(m.CDF_E_star, float).reshape(-1, m.n_lambda)[:, lam - 1]     # (0:n_stars) of this wavelength
    return factor * np.diff(cdf)


def sed_flux(m, sed_mc, n_sent):
    """Monte Carlo SED per packet energy: sed(lambda) * E_totale(lambda) / n_phot_envoyes(lambda), the factor the
    reference applies when it writes sed2 (output.f90: ecriture_sed), without the unit constants."""
    E_tot = np.asarray(m.E_stars) + np.asarray(m.extra["E_disk"])
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(n_sent > 0, E_tot / n_sent, 0.0)
    return sed_mc * f


def image(backend, m, Tdust, lam, n_photons_image, npix_x, npix_y, map_size, zoom=1.0, seed=1, n_chunks=None, method=1,
          ang_disque=0.0, tau_surface=None):
    """One wavelength of ``run_image_mc`` (dust_transfer.f90:692-824): ``repartition_energie(lambda)`` (:737), the image-mode
    packet loop (:748; ``n_photons_image`` packets per stream), then per observer (:775-801) the source function and
    ``dust_map``'s pixels -- ``init_dust_source_fct1`` + RT method 1 for every (ibin, iaz), or ``init_dust_source_fct2`` +
    method 2 per inclination (iaz = 1, 2D) -- with ``compute_stars_map``'s discs added to Stokes I (``dust_map`` :1582-1590)
    and, with ``tau_surface``, the maps of ``compute_tau_map`` / ``compute_tau_surface_map``.
    Returns ``image`` (N_type_flux, nRT, npix_y, npix_x; q = ibin - 1 + RT_n_incl (iaz - 1)), ``stars`` (nRT, npix_y,
    npix_x), ``n_sent`` and, if asked, ``tau_map`` / ``tau_surface_map``."""
    rt = m.rt
    nRT, n_incl, ntf = rt["RT_n_incl"] * rt["RT_n_az"], rt["RT_n_incl"], rt["N_type_flux"]
    if hasattr(backend, "repartition_energie"):
        E_disk = backend.repartition_energie(lam, Tdust)
    else:
        M.repartition_energie(m, Tdust)
        E_disk = float(m.extra["E_disk"][lam - 1])
    r = backend.run_image_mc(lam, int(n_photons_image), seed, n_chunks, method)
    img = np.zeros((ntf, nRT, npix_y, npix_x))
    if method == 1:
        d = np.asarray(backend.dust_image(lam, Tdust, r, E_disk, npix_x, npix_y, map_size, zoom, ang_disque))
        img[:] = d.reshape(ntf, nRT, npix_y, npix_x)           # (N_type_flux, RT_n_az, RT_n_incl, ...): q = ibin-1 + n_incl (iaz-1)
    else:
        if rt["RT_n_az"] != 1 or m.cfg.l3D:
            raise ValueError("ray tracing method 2: 2D grids, one observer azimuth (dust_transfer.f90:789-791)")
        for ibin in range(1, n_incl + 1):
            img[:, ibin - 1] = np.asarray(backend.dust_image_method2(lam, ibin, Tdust, r, E_disk, npix_x, npix_y, map_size, zoom)).reshape(ntf, npix_y, npix_x)
    stars = np.asarray(backend.stars_image(lam, stars_flux_factor(m, lam), npix_x, npix_y, map_size, zoom, seed + 7919 * lam,
                                           ang_disque))[:, 0]
    img[0] += stars
    out = dict(image=img, stars=stars, n_sent=r["n_sent"][lam - 1], E_disk=E_disk)
    if tau_surface is not None:
        out["tau_map"], out["tau_surface_map"] = backend.tau_maps(lam, npix_x, npix_y, map_size, zoom, float(tau_surface), ang_disque)
    return out



def column_maps(backend, m, type, lam=None, gas_density=None, abundance=None):
    """``write_column``'s array (output.f90:1469-1540): ``compute_column`` (optical_depth.f90:328-415) in the shape the file
    gets (:1504-1524) -- ``(4, nz, n_rad)`` on a 2D grid, ``(4, n_az, 2 nz, n_rad)`` in 3D, ``(4, n_cells)`` on a Voronoi grid
    (the FITS axes reversed: C order); index 0 = towards the star, 1 = +z, 2 = -z, 3 = +r.  ``type`` 1: the gas column density
    (g cm^-2; ``gas_density`` in particles m^-3), 2: the dust optical depth at wavelength ``lam`` (1-based), 3: a molecule's
    column density (particles cm^-2; ``abundance``)."""
    col = np.asarray(backend.column(type, lam=lam, gas_density=gas_density, abundance=abundance), np.float32)
    g = m.grid
    if g.get("grid_type", 1) == 3:
        return col.reshape(4, m.n_cells)
    if g["l3D"]:
        return col.reshape(4, g["n_az"], 2 * g["nz"], g["n_rad"])
    return col.reshape(4, g["nz"], g["n_rad"])


def line_map(backend, m, mol, method=2, npix_x=1, npix_y=1, map_size=None, zoom=1.0, ang_disque=0.0, l_sym_ima=False,
             lonly_top=False, lonly_bottom=False):
    """A molecule's line cube and continuum (``emission_line_map``, mol_transfer.f90:484-687, without the stars' maps) in the
    shapes of the files (``ecriture_spectre``: lines.fits.gz and its continuum extension, FITS axes reversed: C order):
    ``spectrum (RT_n_az, RT_n_incl, nTrans, n_speed, npix_y, npix_x)`` and ``continu (RT_n_az, RT_n_incl, nTrans, npix_y,
    npix_x)``, default reals.  ``mol``: ``mcfost_amd.host.molecule.line_tables``.  ``method`` 1: the pixel axes are 1 x 1."""
    if method == 1:
        npix_x = npix_y = 1
    spec, cont = backend.line_map(mol, method=method, npix_x=npix_x, npix_y=npix_y, map_size=map_size, zoom=zoom,
                                  ang_disque=ang_disque, l_sym_ima=l_sym_ima, lonly_top=lonly_top, lonly_bottom=lonly_bottom)
    n_incl, n_az = m.rt["RT_n_incl"], m.rt["RT_n_az"]
    nT, ns = np.asarray(mol["transfreq"]).size, np.asarray(mol["tab_speed"]).size
    return (np.asarray(spec, np.float32).reshape(n_az, n_incl, nT, ns, npix_y, npix_x),
            np.asarray(cont, np.float32).reshape(n_az, n_incl, nT, npix_y, npix_x))


def integ_tau(backend, m, lam, angle):
    """``integ_tau`` (optical_depth.f90:186-244): the optical depths at wavelength ``lam`` (1-based) from the origin along the
    midplane and at ``angle`` degrees from the axis, and next to each the column density (g cm^-2) the reference prints
    (:216-221, :234-239): tau x the dust density of the first non-empty cell over its opacity.  The densities come from the
    model's ``dust_mass`` / ``volume`` (or its ``rho_dust``); ``None`` where the model has neither, with variable dust, or
    where that cell is transparent."""
    tau_mid, tau_ang = backend.integ_tau(lam, angle)
    out = dict(tau_midplane=np.float32(tau_mid), tau_angle=np.float32(tau_ang), column_midplane=None, column_angle=None)
    icell = m.extra.get("icell_ref") if isinstance(getattr(m, "extra", None), dict) else None
    if icell is None or getattr(m, "variable_dust", None) is not None:
        return out
    i = int(icell) - 1
    if "dust_mass" in m.grid:
        rho = float(np.asarray(m.grid["dust_mass"], np.float64)[i]) / (float(np.asarray(m.grid["volume"], np.float64)[i]) * M.AU_TO_CM ** 3)
    elif getattr(m, "rho_dust", None) is not None:
        rho = float(np.asarray(m.rho_dust, np.float64)[i])      # g cm^-3 = dust_mass / (volume AU_to_cm^3)
    else:
        return out
    opacity = float(m.kappa[lam - 1]) * float(np.asarray(m.kappa_factor, np.float64)[i])
    if opacity > M.TINY_REAL:
        out["column_midplane"] = np.float32(float(tau_mid) * rho / (opacity / M.AU_TO_CM))
        out["column_angle"] = np.float32(float(tau_ang) * rho / (opacity / M.AU_TO_CM))
    return out
