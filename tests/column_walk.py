"""The specification the device's column kernels are held to: compute_column's loop (optical_depth.f90:350-411) and
integ_tau's two rays (:186-244, through optical_length_tot :248-324), restated over the ORACLE'S OWN operators --
Oracle.cross_cell / cross_voronoi, Oracle.test_exit_grid, Oracle.index_cell / index_cell_voronoi (oracle/binding.py), which
tests/test_ref_geometry.py pins to the reference's module.  No geometry of its own: the only grid test written out here is
test_exit_grid_Voronoi, `icell < 0` (Voronoi.f90:1446), which the oracle inlines in its operator table and does not export.

All rays of a grid are held in arrays and the live ones advance one cell per iteration.  The geometry of a ray does not
depend on what is summed, so a grid is walked ONCE (`walk_paths`) and the sums of every type and wavelength are formed from
the recorded (cell, l_contrib) steps in the order of the walk (`column_from_paths`): sum = sum + l_contrib * factor in
double, the result a default real.

With variable dust the factor of type 2 takes the class of the CURRENT cell (the reference reads the previous cell's row,
:386-388: a defect, include/mcgpu.h)."""
import numpy as np

AU_TO_M = 149597870700.0
MU_MH = np.float32(float(np.float32(2.3)) * (1.007825032231 * (1.0 / 6.022140857e23)))   # real :: mu_mH = mu * mH
M_TO_CM = 1.0e2


def cd_units(type):
    """(:343-347)"""
    if type == 1:
        return AU_TO_M * float(MU_MH) / M_TO_CM ** 2
    return AU_TO_M / M_TO_CM ** 2


def cell_centres(m):
    """(x1, y1, z1) of every cell (:358-366)."""
    g = m.grid
    n = m.n_cells
    if g.get("grid_type", 1) == 3:
        xyz = np.asarray(g["v_xyz_dp"], np.float64).reshape(-1, 3)[:n]
        return xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy()
    r, z, phi = (np.asarray(g[k], np.float64)[:n] for k in ("r_grid", "z_grid", "phi_grid"))
    return r * np.cos(phi), r * np.sin(phi), z.copy()


def directions(x1, y1, z1):
    """u, v, w [4, n] and ok [4, n] (:368-379); a centre at the origin (1) or on the axis (4) has no direction."""
    n = x1.size
    u, v, w = np.zeros((4, n)), np.zeros((4, n)), np.zeros((4, n))
    ok = np.ones((4, n), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        n2 = x1 * x1 + y1 * y1 + z1 * z1
        ok[0] = n2 > 0.0
        norm = np.where(ok[0], 1.0 / np.sqrt(np.where(ok[0], n2, 1.0)), 0.0)
        u[0], v[0], w[0] = -x1 * norm, -y1 * norm, -z1 * norm
        w[1] = 1.0
        w[2] = -1.0
        n2 = x1 ** 2 + y1 ** 2
        ok[3] = n2 > 0.0
        norm = np.where(ok[3], 1.0 / np.sqrt(np.where(ok[3], n2, 1.0)), 0.0)
        u[3], v[3] = x1 * norm, y1 * norm
    return u, v, w, ok


def _walk(o, m, x, y, z, u, v, w, cell, live, max_steps):
    """Advances the live rays from (x, y, z) in `cell` (previous_cell = 0) to the edge of the grid.  Returns the steps:
    a list of (ray indices, icell0, l_contrib) per iteration, and the number of rays still live after max_steps."""
    voro = m.grid.get("grid_type", 1) == 3
    n_cells = m.n_cells
    x, y, z = x.copy(), y.copy(), z.copy()
    nxt = np.asarray(cell, np.int32).copy()
    cur = np.zeros_like(nxt)
    live = live.copy()
    steps = []
    for _ in range(max_steps):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        prev = cur[idx].copy()
        cur[idx] = nxt[idx]
        c = cur[idx]
        out = (c < 0) if voro else o.test_exit_grid(c, x[idx], y[idx], z[idx]).astype(bool)
        live[idx[out]] = False
        idx, c, prev = idx[~out], c[~out], prev[~out]
        if idx.size == 0:
            break
        if voro:
            r = o.cross_voronoi(x[idx], y[idx], z[idx], u[idx], v[idx], w[idx], c, prev)
            x1, y1, z1, nc, lc = r["x1"], r["y1"], r["z1"], r["next_cell"], r["l_contrib"]
        else:
            x1, y1, z1, nc, lc = o.cross_cell(x[idx], y[idx], z[idx], u[idx], v[idx], w[idx], c)   # (l_contrib = l)
        real = c <= n_cells
        steps.append((idx[real], c[real].astype(np.int64), np.asarray(lc, np.float64)[real]))
        x[idx], y[idx], z[idx], nxt[idx] = x1, y1, z1, nc
    return steps, int(live.sum())


def walk_paths(o, m, max_steps=100000):
    """compute_column's rays of a grid, t = direction * n_cells + (icell - 1): dict(steps, n_rays, ok, n_steps, unfinished)."""
    n = m.n_cells
    x1, y1, z1 = cell_centres(m)
    u, v, w, ok = directions(x1, y1, z1)
    cell = np.tile(np.arange(1, n + 1, dtype=np.int32), 4)
    steps, left = _walk(o, m, np.tile(x1, 4), np.tile(y1, 4), np.tile(z1, 4), u.reshape(-1), v.reshape(-1), w.reshape(-1),
                        cell, ok.reshape(-1), max_steps)
    n_steps = np.zeros(4 * n, np.int64)
    for idx, _, _ in steps:
        n_steps[idx] += 1
    return dict(steps=steps, n_rays=4 * n, ok=ok.reshape(-1), n_steps=n_steps, unfinished=left)


def type2_factor(m, lam, kappa_factor=None):
    """kappa(p_icell, lambda) * kappa_factor(icell0) per cell, the class of the cell itself with variable dust."""
    kf = np.asarray(m.kappa_factor if kappa_factor is None else kappa_factor, np.float64)
    vd = getattr(m, "variable_dust", None)
    if vd is None:
        return float(np.asarray(m.kappa, np.float64)[lam - 1]) * kf
    nc = int(vd["p_n_cells"])
    kap = np.asarray(vd["kappa"], np.float64).reshape(m.n_lambda, nc)[lam - 1]
    return kap[np.asarray(vd["p_icell"], np.int64) - 1] * kf


def factor_of(m, type, lam=None, gas_density=None, abundance=None, kappa_factor=None):
    """`factor` of every cell in the reference's order of operations (:397-403)."""
    if type == 2:
        return type2_factor(m, lam, kappa_factor)
    f = cd_units(type) * np.asarray(gas_density, np.float64)
    if type == 3:
        f = f * np.asarray(abundance, np.float32).astype(np.float64)
    return f


def column_from_paths(paths, factor):
    """column [4, n_cells] float32 from the recorded steps: sum = sum + l_contrib * factor, in the walk's order."""
    s = np.zeros(paths["n_rays"], np.float64)
    for idx, c, lc in paths["steps"]:
        s[idx] = s[idx] + lc * factor[c - 1]
    return s.astype(np.float32).reshape(4, -1)


def integ_tau_directions(angle_deg):
    """(:205, :225-227): angle is a default real."""
    w0 = float(np.cos(np.float64(np.float32(angle_deg)) * np.pi / 180.0))
    return np.array([1.0, np.sqrt(1.0 - w0 * w0)]), np.zeros(2), np.array([0.0, w0])


def integ_tau_walk(o, m, lam, angle_deg, max_steps=100000):
    """(tau_midplane, tau_angle) as default reals: index_cell at the origin, then optical_length_tot's loop."""
    u, v, w = integ_tau_directions(angle_deg)
    z0 = np.zeros(2)
    voro = m.grid.get("grid_type", 1) == 3
    cell = o.index_cell_voronoi(z0, z0, z0) if voro else o.index_cell(z0, z0, z0)
    steps, left = _walk(o, m, z0, z0, z0, u, v, w, cell, np.ones(2, bool), max_steps)
    assert left == 0
    f = type2_factor(m, lam)
    s = np.zeros(2)
    for idx, c, lc in steps:
        s[idx] = s[idx] + lc * f[c - 1]
    return np.float32(s[0]), np.float32(s[1])
