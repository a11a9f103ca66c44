"""TEST INFRASTRUCTURE: a plain numpy restatement of the reference's routines for the grains in radiative equilibrium out
of LTE, written from the reference's lines, sequential sums included -- the yardstick of tests/test_nlte*.py:

  im_reemission_NLTE   thermal_emission.f90:775-866     reemission_nlte()
  Temp_finale_nLTE     thermal_emission.f90:932-1014    temp_finale_nlte()
  repartition_energie  thermal_emission.f90:1832-1850   repartition_nlte_term()

Arrays are C-ordered with the Fortran first index last, as ``mcfost_amd.host.model.init_nlte`` returns them.  Events are
vectorised ACROSS events only: every event's own sums and searches run in the reference's order."""
import numpy as np

f64 = np.float64


def j_abs(C_abs_norm, J, k, ic):
    """J_abs = sum over lambda, in order, of C_abs_norm(k, lambda) * J(icell, lambda)  (:813-816; J = xJ_abs + J0)"""
    out = np.zeros(k.shape, f64)
    for l in range(C_abs_norm.shape[0]):
        out = out + C_abs_norm[l, k - 1].astype(f64) * J[l, ic - 1]
    return out


def search_T(lE, k, log_E_abs):
    """the ratchet from its initial value 2 (:823-828): while (log_E_em_1grain(k,T_int) < log_E_abs .and. T_int < n_T)"""
    n_T = lE.shape[0]
    T_int = np.full(k.shape, 2, np.int64)
    while True:
        go = (lE[T_int - 1, k - 1] < log_E_abs) & (T_int < n_T)
        if not go.any():
            return T_int
        T_int = T_int + go


def interp_temp(lE, tab_Temp, k, T_int, log_E_abs):
    """:833-838"""
    Temp2 = tab_Temp[T_int - 1].astype(f64)
    Temp1 = tab_Temp[T_int - 2].astype(f64)
    lE1, lE2 = lE[T_int - 2, k - 1], lE[T_int - 1, k - 1]
    with np.errstate(all="ignore"):
        frac = (log_E_abs - lE1) / (lE2 - lE1)
        Temp = np.exp(np.log(Temp2) * frac + np.log(Temp1) * (1.0 - frac))
    return Temp, Temp1, Temp2


def reemission_nlte(nl, tab_Temp, volume, L_packet_th, icell, lambda0, rand1, rand2, J=None, shift=0.0):
    """im_reemission_NLTE for arrays of events (icell, lambda0 1-based; rand1, rand2 default real).  ``J [n_lambda, n_cells]``:
    xJ_abs summed over threads + J0 (default: nl["J0"]).  ``shift``: log_E_abs is multiplied by (1 + shift) before the
    searches (the stability rule of the tests).  Returns (k, T_int, Temp, lambda, log_E_abs)."""
    C, kcdf, lE, cdf = nl["C_abs_norm"], nl["kabs_nLTE_CDF"], nl["log_E_em_1grain"], nl["kdB_dT_1grain_nLTE_CDF"]
    J = nl["J0"] if J is None else J
    n, n_lambda = int(nl["n_grains"]), C.shape[0]
    icell, lambda0 = np.asarray(icell, np.int64), np.asarray(lambda0, np.int64)
    r1, r2 = np.asarray(rand1, np.float32).astype(f64), np.asarray(rand2, np.float32).astype(f64)
    # the grain: kmin = grain_RE_nLTE_start, kmax = grain_RE_nLTE_end (1 .. n here), :798-810
    kmin = np.full(icell.shape, 1, np.int64)
    kmax = np.full(icell.shape, n, np.int64)
    k = (kmin + kmax) // 2
    while True:
        go = (kmax - kmin) > 1
        if not go.any():
            break
        less = kcdf[lambda0 - 1, k] < r1
        kmin = np.where(go & less, k, kmin)
        kmax = np.where(go & ~less, k, kmax)
        k = (kmin + kmax) // 2
    k = kmax
    with np.errstate(all="ignore"):
        log_E_abs = np.log(j_abs(C, J, k, icell) * L_packet_th / volume[icell - 1]) * (1.0 + shift)
    T_int = search_T(lE, k, log_E_abs)
    Temp, Temp1, Temp2 = interp_temp(lE, tab_Temp, k, T_int, log_E_abs)
    frac_T2 = (Temp - Temp1) / (Temp2 - Temp1)
    frac_T1 = 1.0 - frac_T2
    l1 = np.zeros(icell.shape, np.int64)
    l2 = np.full(icell.shape, n_lambda, np.int64)
    l = (l1 + l2) // 2
    while True:
        go = (l2 - l1) > 1
        if not go.any():
            break
        lc = np.maximum(l, 1)
        proba = frac_T1 * cdf[T_int - 2, k - 1, lc - 1] + frac_T2 * cdf[T_int - 1, k - 1, lc - 1]
        up = r2 > proba
        l1 = np.where(go & up, l, l1)
        l2 = np.where(go & ~up, l, l2)
        l = (l1 + l2) // 2
    return k, T_int, Temp, l + 1, log_E_abs


def unstable_events(nl, tab_Temp, volume, L_packet_th, icell, lambda0, rand1, rand2, J=None, rel=1e-12):
    """events whose T_int or lambda the restatement itself changes when log_E_abs moves by +-rel relative"""
    base = reemission_nlte(nl, tab_Temp, volume, L_packet_th, icell, lambda0, rand1, rand2, J)
    bad = np.zeros(np.asarray(icell).shape, bool)
    for s in (rel, -rel):
        o = reemission_nlte(nl, tab_Temp, volume, L_packet_th, icell, lambda0, rand1, rand2, J, shift=s)
        bad |= (o[1] != base[1]) | (o[3] != base[3])
    return base, bad


def temp_finale_nlte(nl, tab_Temp, volume, L_packet_th, T_min, xJ_abs):
    """Temp_finale_nLTE: Tdust_1grain [n_cells, n] (default real); xJ_abs [n_lambda, n_cells] summed over threads"""
    C, lE = nl["C_abs_norm"], nl["log_E_em_1grain"]
    n, n_cells = int(nl["n_grains"]), volume.size
    J = xJ_abs + nl["J0"] if nl.get("J0") is not None else xJ_abs
    dens = nl.get("grain_density")
    out = np.zeros((n_cells, n), np.float32)
    ic = np.arange(1, n_cells + 1)
    tiny = np.finfo(f64).tiny
    for kk in range(1, n + 1):
        k = np.full(n_cells, kk, np.int64)
        J_absorbe = j_abs(C, J, k, ic) * L_packet_th / volume
        with np.errstate(all="ignore"):
            log_E_abs = np.log(J_absorbe)
        T_int = search_T(lE, k, np.where(np.isfinite(log_E_abs), log_E_abs, -1e300))
        Temp, _, _ = interp_temp(lE, tab_Temp, k, T_int, log_E_abs)
        T = np.where((J_absorbe < tiny) | (log_E_abs < lE[0, kk - 1]), np.float32(T_min), Temp.astype(np.float32))
        if dens is not None:
            T = np.where(dens[:, kk - 1] > tiny, T, np.float32(0.0))
        out[:, kk - 1] = T
    return out


def repartition_nlte_term(nl, wl_um, lam_index, Tdust_1grain, volume, dark=None):
    """E_emise(icell) of the lRE_nLTE block (:1832-1850) at wavelength index lam_index (1-based)"""
    thermal_const = float(np.float32(299792458.0 * 6.626070040e-34 / 1.38064852e-23))
    wl = wl_um * float(np.float32(1.0e-6))
    cst_wl_max = float(np.log(np.finfo(np.float32).max)) - float(np.float32(1.0e-4))
    C, dens = nl["C_abs_norm"], nl["grain_density"]
    n_cells, n = Tdust_1grain.shape
    E = np.zeros(n_cells, f64)
    for k in range(n):
        Temp = Tdust_1grain[:, k].astype(f64)
        ok = Tdust_1grain[:, k] > np.finfo(np.float32).tiny
        with np.errstate(all="ignore"):
            cst_wl = thermal_const / (np.where(ok, Temp, 1.0) * wl)
            term = 4.0 * float(C[lam_index - 1, k]) * dens[:, k] * volume / ((wl ** 5) * (np.exp(cst_wl) - 1.0))
        E = E + np.where(ok & (cst_wl < cst_wl_max), term, 0.0)
    if dark is not None:
        E = np.where(np.asarray(dark) != 0, 0.0, E)
    return E
