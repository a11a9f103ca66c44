"""TEST INFRASTRUCTURE shared by tests/test_nlte.py and tests/test_nlte_gpu.py: the model with non-LTE grains and the random
re-emission events both suites check against the restatement (tests/nlte_restatement.py)."""
import dataclasses
import math

import numpy as np

from mcfost_amd.host import model as M

N_TOTAL = 100000       # packets L_packet_th is formed for


def nlte_model(cfg=None, n_grains=16, nlte_range=None, xi=0.0, **kw):
    """(model, nl): ``small()`` with ``synthetic_grains(n_grains)``, grains ``nlte_range`` (default: all) out of LTE; with LTE
    grains left, the model's LTE tables become those of the LTE grains' share (``init_nlte``)."""
    m = M.build_model(cfg if cfg is not None else M.small())
    grains = M.synthetic_grains(m, n_grains)
    _, dens = M.settled_grain_density(m, grains, xi=xi, per_cell=False, n_classes=1)   # (one class; xi = 0: unsettled)
    nl = M.init_nlte(m, grains, dens, nlte_range or (1, n_grains), **kw)
    if nl["Proba_abs_RE_LTE"] is not None:
        m = dataclasses.replace(m, kappa_abs_LTE=nl["kappa_abs_LTE"], log_Qcool=nl["log_Qcool"], kdB_dT_CDF=nl["kdB_dT_CDF"])
    return m, nl


def smooth_field(m, nl, decades_beyond=1.0):
    """J0 [n_lambda, n_cells]: a smooth synthetic field per cell -- a diluted blackbody whose colour temperature and
    amplitude vary from cell to cell so that, over the cells and grains, log_E_abs spans every grain's whole
    log_E_em_1grain row and ``decades_beyond`` decades past each end."""
    lam = np.asarray(m.lam, np.float64)
    n_cells = m.n_cells
    vol = np.asarray(m.grid["volume"], np.float64)[:n_cells]
    L = m.L_packet_th(N_TOTAL)
    Tc = 30.0 * 100.0 ** ((np.arange(n_cells) * 7 % n_cells) / max(1, n_cells - 1))       # 30 .. 3000 K, shuffled
    x = 14387.77 / (lam[:, None] * Tc[None, :])
    shape = 1.0 / (lam[:, None] ** 5 * np.expm1(np.minimum(x, 600.0)))                    # [n_lambda, n_cells]
    shape = shape / shape.max(axis=0)
    C = nl["C_abs_norm"].astype(np.float64)                                               # [n_lambda, n]
    base = np.log((C.T @ shape) * L / vol[None, :])                                       # [n, n_cells] log_E_abs at A = 1
    lE = nl["log_E_em_1grain"]
    lo = (lE[0] - decades_beyond * math.log(10.0))[:, None] - base                        # log A that reaches each end
    hi = (lE[-1] + decades_beyond * math.log(10.0))[:, None] - base
    lo, hi = lo.min(), hi.max()
    logA = lo + (hi - lo) * (np.arange(n_cells) + 0.5) / n_cells
    return np.ascontiguousarray(shape * np.exp(logA)[None, :])


def random_events(m, nl, n, seed=11):
    rng = np.random.default_rng(seed)
    icell = rng.integers(1, m.n_cells + 1, n).astype(np.int32)
    lambda0 = rng.integers(1, m.n_lambda + 1, n).astype(np.int32)
    draw = lambda: (rng.integers(0, 1 << 24, n).astype(np.float32) * np.float32(1.0 / 16777216.0))   # 24-bit uniforms
    return icell, lambda0, draw(), draw()


def compare_events(got, nl, tab_Temp, volume, L, icell, lambda0, r1, r2, max_left_out=1e-4):
    """the rule of the event tests: k and T_int equal, Temp to rtol 1e-12, lambda equal; an event may be left out only if
    the restatement itself changes its T_int or lambda when log_E_abs moves by +-1e-12 relative"""
    from nlte_restatement import unstable_events
    (k, T_int, Temp, lam, log_E), unstable = unstable_events(nl, tab_Temp, volume, L, icell, lambda0, r1, r2)
    n = icell.size
    assert unstable.sum() <= max_left_out * n, int(unstable.sum())
    keep = ~unstable
    gk, gT, gTemp, glam = got
    assert np.array_equal(gk, k), "the grain is drawn before J_abs: no event is left out of this"
    assert np.array_equal(gT[keep], T_int[keep]), int((gT[keep] != T_int[keep]).sum())
    assert np.allclose(gTemp[keep], Temp[keep], rtol=1e-12, atol=0.0)
    assert np.array_equal(glam[keep], lam[keep]), int((glam[keep] != lam[keep]).sum())
    return dict(left_out=int(unstable.sum()), grains=np.unique(k), T_span=(int(T_int.min()), int(T_int.max())), log_E=log_E)
