"""Host arithmetic of the molecular line transfer in LTE, plain numpy: the arrays the reference fills before it calls
``emission_line_map`` and that ``mcgpu_line_map`` (include/mcgpu.h) takes as its input.

Restated from the reference, in its precisions (a ``real`` is a float32, a ``real(kind=dp)`` a float64):
  init_doppler_profiles  init_Doppler_profiles  (molecular_emission.f90:141-179)
  equilibre_lte_mol      equilibre_LTE_mol      (:372-425)
  opacite_mol_loc        opacite_mol_loc        (:305-337, with the clamp of an inverted population at 0)
  tab_speed_rt           span(vmin, vmax, n)    (mol_transfer.f90:531; utils.f90:43-62, accumulated in single precision)
  einstein               Aul -> Bul -> Blu and the f* products (input.f90:138-146)
An INPUT, like ``model.synthetic_dust``, not a restatement: ``linear_rotor`` (levels, weights, Aul and frequencies of a
rigid linear rotor in closed form, CO-like by default) and ``dust_at_transitions`` (the dust's opacity and thermal
emissivity at the lines' frequencies from the model's tables).  ``line_tables`` puts them together for a model's temperatures.
Non-LTE populations (equilibre_rad_mol_loc and the iterations around it) stay with the host code that owns them: hand their
tab_nLevel to ``opacite_mol_loc``."""
import numpy as np

f32, f64 = np.float32, np.float64
HP = 6.626070040e-34
KB = 1.38064852e-23
C_LIGHT = 299792458.0
AU_TO_M = 149597870700.0
MH = 1.007825032231 * (1.0 / 6.022140857e23)   # g (constants.f90)
G_TO_KG = 1.0e-3
PI = np.pi


def linear_rotor(n_levels=8, B_GHz=57.635968, mu_debye=0.11011, molecular_weight=28.0, name="CO-like rotor"):
    """A rigid linear rotor: level l = J + 1, g = 2 J + 1, transition J -> J - 1 at 2 B J with the dipole's Aul.
    Transition l - 1 connects the levels l and l - 1, as equilibre_LTE_mol assumes."""
    J = np.arange(n_levels)
    g = (2.0 * J + 1.0).astype(f32)                                # real stat_weight_g
    Ju = np.arange(1, n_levels, dtype=f64)
    freq = 2.0 * B_GHz * 1.0e9 * Ju                               # Hz
    mu_SI = mu_debye * 3.33564e-30
    eps0 = 8.8541878128e-12
    A = 16.0 * PI ** 3 * freq ** 3 * mu_SI ** 2 / (3.0 * eps0 * HP * C_LIGHT ** 3) * Ju / (2.0 * Ju + 1.0)
    return dict(name=name, n_levels=int(n_levels), stat_weight_g=g, transfreq=freq, Aul=A,
                itransUpper=np.arange(2, n_levels + 1), itransLower=np.arange(1, n_levels), molecularWeight=f32(molecular_weight))


def einstein(rotor):
    """fAul, fBul, fBlu (input.f90:138-146)."""
    g = np.asarray(rotor["stat_weight_g"], f32)
    fr, A = np.asarray(rotor["transfreq"], f64), np.asarray(rotor["Aul"], f64)
    Bul = A * (C_LIGHT ** 2) / (2.0 * HP * fr ** 3)
    up, lo = np.asarray(rotor["itransUpper"]) - 1, np.asarray(rotor["itransLower"]) - 1
    Blu = Bul * (g[up] / g[lo]).astype(f64)                        # (a quotient of reals)
    k = HP * fr / (4 * PI)
    return A * k, Bul * k, Blu * k


def tab_speed_rt(vmin, vmax, n):
    """span(vmin, vmax, n) in m/s as real(dp): a default-real delta added n - 1 times in single precision."""
    vmin, vmax = f32(vmin), f32(vmax)
    out = np.empty(n, f32)
    delta = f32((vmax - vmin) / f32(n - 1)) if n > 1 else f32(0)
    out[0] = vmin
    for i in range(1, n):
        out[i] = f32(out[i - 1] + delta)
    return out.astype(f64)


def init_doppler_profiles(Tcin, molecular_weight, v_turb2):
    """dv_line (real), sigma2_phiProf_m1, norme_phiProf_m1 (dp) per cell."""
    T = np.asarray(Tcin, f32).astype(f64)
    vt2 = np.broadcast_to(np.asarray(v_turb2, f32), T.shape).astype(f64)
    sigma2 = 2.0 * (KB * T / (float(f32(molecular_weight)) * MH * G_TO_KG)) + vt2
    return dict(dv_line=np.sqrt(sigma2).astype(f32), sigma2_phiProf_m1=1.0 / sigma2,
                norme_phiProf_m1=C_LIGHT / np.sqrt(PI * sigma2))


def equilibre_lte_mol(rotor, Tcin, gas_density, tab_abundance):
    """tab_nLevel [n_cells, n_levels] (real): Boltzmann populations at Tcin, normalised to gas_density * tab_abundance."""
    T = np.asarray(Tcin, f32).astype(f64)
    g = np.asarray(rotor["stat_weight_g"], f32)
    fr = np.asarray(rotor["transfreq"], f64)
    nl = int(rotor["n_levels"])
    pop = np.zeros((T.size, nl), f32)
    pop[:, 0] = 1.0
    for l in range(1, nl):
        ratio = (pop[:, l - 1] * g[l] / g[l - 1]).astype(f64)      # real * real / real
        pop[:, l] = (ratio * np.exp(-HP * fr[l - 1] / (KB * T))).astype(f32)
    tot = np.zeros(T.size, f32)
    for l in range(nl):                                            # sum(pop_levels): a real
        tot = (tot + pop[:, l]).astype(f32)
    norm = np.asarray(gas_density, f64) * np.asarray(tab_abundance, f32).astype(f64) / tot.astype(f64)
    return (pop.astype(f64) * norm[:, None]).astype(f32)


def opacite_mol_loc(rotor, tab_nLevel, transitions):
    """(kappa_mol_o_freq, emissivite_mol_o_freq) [nTrans, n_cells] for the 1-based ``transitions``."""
    fA, fBul, fBlu = einstein(rotor)
    fr = np.asarray(rotor["transfreq"], f64)
    n = np.asarray(tab_nLevel, f32).astype(f64)
    kap_out, eps_out = [], []
    for t in transitions:
        i = int(t) - 1
        nu, nl = n[:, int(rotor["itransUpper"][i]) - 1], n[:, int(rotor["itransLower"][i]) - 1]
        kap = nl * fBlu[i] - nu * fBul[i]
        kap = np.where(kap < 0.0, 0.0, kap)
        kap_out.append(kap / fr[i] * AU_TO_M)
        eps_out.append(nu * fA[i] / fr[i] * AU_TO_M)
    return np.array(kap_out), np.array(eps_out)


def dust_at_transitions(m, transfreq, Tdust):
    """(kappa_abs_LTE [nTrans, p_n_cells], emissivite_dust [nTrans, n_cells]) at the lines: the model's absorption opacity
    (AU^-1 at the reference cell) interpolated in log wavelength, and kappa_abs * kappa_factor * B_nu(Tdust) in SI."""
    lam = np.asarray(m.lam, f64)
    wl_um = C_LIGHT / np.asarray(transfreq, f64) * 1.0e6
    vd = getattr(m, "variable_dust", None)
    if vd is None:
        rows = np.asarray(m.kappa_abs_LTE, f64)[None, :]
        cls = np.zeros(m.n_cells, np.int64)
    else:
        nc = int(vd["p_n_cells"])
        rows = np.asarray(vd["kappa_abs_LTE"] if "kappa_abs_LTE" in vd else vd["kappa"], f64).reshape(m.n_lambda, nc).T
        cls = np.asarray(vd["p_icell"], np.int64) - 1
    kabs = np.array([[np.exp(np.interp(np.log(w), np.log(lam), np.log(np.maximum(r, 1e-300)))) for r in rows] for w in wl_um])
    T = np.maximum(np.asarray(Tdust, f64), 1.0)
    fr = np.asarray(transfreq, f64)[:, None]
    Bnu = 2.0 * HP * fr ** 3 / C_LIGHT ** 2 / np.expm1(HP * fr / (KB * T[None, :]))
    emis = kabs[:, cls] * np.asarray(m.kappa_factor, f64)[None, :] * Bnu
    return kabs, emis


def line_tables(m, rotor, Tdust, gas_density, tab_abundance, transitions, tab_speed, v_turb=0.0, velocity=None):
    """The input of ``Engine.line_map`` / ``mcgpu_line_map`` for the 1-based ``transitions`` of ``rotor`` with the dust
    temperature as the kinetic one.  ``velocity``: the entries of the velocity field (vfield_mode, vfield, lkeplerian,
    linfall, chi_infall, vfield_coord, vxyz), merged into the result."""
    T = np.asarray(Tdust, f32)[:m.n_cells]
    prof = init_doppler_profiles(T, rotor["molecularWeight"], f32(v_turb) * f32(v_turb))
    pops = equilibre_lte_mol(rotor, T, gas_density, tab_abundance)
    kap, eps = opacite_mol_loc(rotor, pops, transitions)
    fr = np.asarray(rotor["transfreq"], f64)[np.asarray(transitions, np.int64) - 1]
    kabs, edust = dust_at_transitions(m, fr, T)
    out = dict(tab_speed=np.asarray(tab_speed, f64), transfreq=fr, kappa_mol_o_freq=kap, emissivite_mol_o_freq=eps,
               emissivite_dust=edust, kappa_abs_LTE=kabs, tab_nLevel=pops, **prof)
    out.update(velocity or {})
    return out


def keplerian_vfield(m, mstar_msun=1.0):
    """vfield [n_cells] (real): the Keplerian speed at the cell's cylindrical radius, m/s."""
    g = m.grid
    r = np.asarray(g["r_grid"], f64)[:m.n_cells]
    GM = 6.67408e-11 * 1.98855e30 * mstar_msun
    return np.sqrt(GM / (np.maximum(r, 1e-30) * AU_TO_M)).astype(f32)
