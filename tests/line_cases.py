"""Shared by tests/test_line_map.py and tests/test_line_map_gpu.py: the cases of the line ray tracer -- the five grids of
tests/column_cases.py::GRIDS, each with a velocity field, two inclinations (one near edge-on; two azimuths on cyl3d), two
transitions of the synthetic rotor and 33 or 81 channels -- with the walk of each view (tests/line_walk.py) and the
restatement's cubes, computed once per session and left unchanged.

Temperatures are the model's own: a short temperature step of the CPU oracle.  The tables come from
mcfost_amd/host/molecule.py.  Seeds, the turbulent width and the cold case's temperature scale were chosen so that in every
case dv / dv_line * 20 stays further than 1e-4 from a half-integer at every step (tests/test_line_map.py asserts it): n_vpoints
is then the same in every build of the arithmetic."""
import functools

import numpy as np

import column_cases as K
import line_walk as W
from mcfost_amd.host import model as M
from mcfost_amd.host import molecule as MOL
from oracle import Oracle

RTOL = K.RTOL            # default-real results of ray walks
ATOL_REL = 1e-8          # x the cube's largest value (helpers.xI_close)
NPIX = 12
TRANSITIONS = (2, 3)     # J = 2-1 and 3-2 of the rotor
VMAX = 6000.0            # m/s
N_SPEEDS = (33, 81)      # 81: one full pass of 64 lanes and a remainder of 17

# name -> (grid, velocity field, options of the tables)
CASES = {
    "cyl2d": ("cyl2d", "kepler", dict(v_turb=200.0)),
    "cyl2d_cold": ("cyl2d", "kepler", dict(v_turb=0.0, T_scale=0.02)),
    "cyl3d": ("cyl3d", "kepler_infall", dict(v_turb=200.0)),
    "sph2d": ("sph2d", "file2", dict(v_turb=200.0, seed=6)),
    "sph3d_v3": ("sph3d", "file3", dict(v_turb=200.0)),
    "sph3d_v1": ("sph3d", "file1", dict(v_turb=200.0)),
    "voronoi": ("voronoi", "vxyz", dict(v_turb=200.0)),
}


@functools.lru_cache(maxsize=None)
def grid_case(grid):
    """(model, oracle, Tdust, rays, paths) of a grid: the model with its two inclinations, its temperatures, the view walked."""
    more = dict(RT_imin=40.0, RT_imax=87.0, RT_n_incl=2)
    if grid == "cyl3d":
        more.update(RT_n_az=2, RT_az_min=0.0, RT_az_max=60.0)
    m = K.build(grid, **more)
    o = Oracle(m, 20000)
    T = np.asarray(o.temp_finale(o.run_thermal(20000, seed=3, n_threads=1)["E_abs"]), np.float32)[:m.n_cells]
    rays = W.ray_starts(m, 2, NPIX, NPIX, map_size(m))
    paths = W.walk_paths(o, m, rays)
    assert paths["unfinished"] == 0
    return m, o, T, rays, paths


def map_size(m):
    return 2.2 * float(m.cfg.rout)


def centres_xyz(m):
    g = m.grid
    n = m.n_cells
    if g.get("grid_type", 1) == 3:
        xyz = np.asarray(g["v_xyz_dp"], np.float64).reshape(-1, 3)[:n]
        return xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r, z, phi = (np.asarray(g[k], np.float64)[:n] for k in ("r_grid", "z_grid", "phi_grid"))
    return r * np.cos(phi), r * np.sin(phi), z


def kepler_speed(m):
    x, y, _ = centres_xyz(m)
    GM = 6.67408e-11 * 1.98855e30
    return np.sqrt(GM / (np.maximum(np.hypot(x, y), 1e-3) * MOL.AU_TO_M))


def velocity(m, kind, seed=5):
    """The entries of the velocity field of a case."""
    n = m.n_cells
    vk = kepler_speed(m)
    rng = np.random.default_rng(seed)
    if kind == "kepler":
        return dict(vfield_mode=1, vfield=vk.astype(np.float32), lkeplerian=True, linfall=False)
    if kind == "kepler_infall":
        return dict(vfield_mode=1, vfield=vk.astype(np.float32), lkeplerian=True, linfall=True, chi_infall=np.float32(0.3))
    if kind == "vxyz":
        x, y, _ = centres_xyz(m)
        r = np.maximum(np.hypot(x, y), 1e-3)
        return dict(vxyz=np.stack([-y / r * vk, x / r * vk, np.zeros(n)], 1).reshape(-1))
    if kind in ("file2", "file3"):                  # (v_r, v_phi, v_z or v_theta): rotation and seeded motions
        comp = [300.0 * rng.normal(size=n), vk * (1.0 + 0.05 * rng.normal(size=n)), 200.0 * rng.normal(size=n)]
        return dict(vfield_mode=2, vfield_coord=int(kind[-1]), vfield=np.array(comp, np.float32).reshape(-1))
    x, y, _ = centres_xyz(m)                         # file1: Cartesian, constant in a cell
    r = np.maximum(np.hypot(x, y), 1e-3)
    comp = [-y / r * vk + 300.0 * rng.normal(size=n), x / r * vk + 300.0 * rng.normal(size=n), 200.0 * rng.normal(size=n)]
    return dict(vfield_mode=2, vfield_coord=1, vfield=np.array(comp, np.float32).reshape(-1))


def gas_and_abundance(m):
    """gas_density (particles m^-3, gas to dust 100) and a uniform tab_abundance"""
    mu_mH = 2.3 * MOL.MH
    return np.asarray(m.rho_dust, np.float64)[:m.n_cells] * 100.0 / mu_mH * 1.0e6, np.full(m.n_cells, 1.0e-4, np.float32)


def tables(name, n_speed, tab_speed=None, **override):
    """The molecule's tables of a case (fresh arrays: a test may change them)."""
    grid, kind, opt = CASES[name]
    opt = dict(opt, **override)
    seed = opt.pop("seed", 5)
    m, _, T, _, _ = grid_case(grid)
    gas, ab = gas_and_abundance(m)
    ts = MOL.tab_speed_rt(-VMAX, VMAX, n_speed) if tab_speed is None else np.asarray(tab_speed, np.float64)
    Tk = (T.astype(np.float64) * opt.get("T_scale", 1.0)).astype(np.float32)
    return MOL.line_tables(m, MOL.linear_rotor(), Tk, gas, ab, TRANSITIONS, ts, v_turb=opt["v_turb"], velocity=velocity(m, kind, seed))


@functools.lru_cache(maxsize=None)
def case(name, n_speed):
    """(model, oracle, tables, the restatement's result) of a case"""
    m, o, _, rays, paths = grid_case(CASES[name][0])
    mol = tables(name, n_speed)
    return m, o, mol, W.cube_from_paths(m, mol, rays, paths)


def compare(got, want, what):
    """The same zero pattern, rtol 2e-6 and atol 1e-8 x the largest value; returns the largest relative difference among the
    values above the atol."""
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(got != 0, want != 0), what
    atol = ATOL_REL * float(np.abs(want).max())
    assert np.allclose(got, want, rtol=RTOL, atol=atol), (what, float(np.max(np.abs(got.astype(np.float64) - want))))
    big = np.abs(want) > atol
    return float(np.max(np.abs(got[big].astype(np.float64) - want[big]) / np.abs(want[big]))) if big.any() else 0.0
