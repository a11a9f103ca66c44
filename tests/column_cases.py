"""Shared by tests/test_column.py and tests/test_column_gpu.py: the grids, their seeded inputs and the walk of each grid
(tests/column_walk.py), computed once per session and left unchanged."""
import functools

import numpy as np

import column_walk as W
from mcfost_amd.host import model as M
from oracle import Oracle

# the five grids of tests/test_tau_maps.py::GRIDS
GRIDS = {
    "cyl2d": dict(),
    "cyl3d": dict(n_rad=12, nz=6, n_az=8, l3D=True),
    "sph2d": dict(grid_type=2),
    "sph3d": dict(grid_type=2, n_rad=10, nz=6, n_az=6, l3D=True),
    "voronoi": dict(voronoi_sites=1200),
}
RTOL = 2e-6   # the project's tolerance for optical depths along rays (tests/test_tau_maps.py::_compare)


def build(name, **more):
    kw = dict(GRIDS[name])
    sites = kw.pop("voronoi_sites", 0)
    kw.update(more)
    return M.build_voronoi_model(M.small(**kw), sites, seed=3) if sites else M.build_model(M.small(**kw))


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, oracle, paths of compute_column's rays) of a grid."""
    m = build(name)
    o = Oracle(m, 1000)
    paths = W.walk_paths(o, m)
    assert paths["unfinished"] == 0
    return m, o, paths


def seeded(m):
    """gas_density (real(dp), part. m^-3) and tab_abundance (default real): seeded log-normal arrays."""
    rng = np.random.default_rng(11)
    gas = 1.0e12 * np.exp(rng.normal(size=m.n_cells))
    ab = (1.0e-4 * np.exp(rng.normal(size=m.n_cells))).astype(np.float32)
    return gas, ab


def wavelengths(m):
    """type 2: wavelength 3 and the wavelength nearest 1 um (1-based)."""
    return 3, int(np.argmin(np.abs(np.asarray(m.lam) - 1.0))) + 1


def centres(m):
    """r_grid, z_grid, phi_grid of a cylindrical or spherical grid; Nones on a Voronoi grid."""
    g = m.grid
    if g.get("grid_type", 1) == 3:
        return None, None, None
    n = m.n_cells
    return tuple(np.ascontiguousarray(np.asarray(g[k], np.float64)[:n]) for k in ("r_grid", "z_grid", "phi_grid"))


def variants(m):
    """(type, lam, gas, abundance) of the comparisons: types 1, 2 (two wavelengths) and 3."""
    gas, ab = seeded(m)
    l1, l2 = wavelengths(m)
    return [(1, None, gas, None), (2, l1, None, None), (2, l2, None, None), (3, None, gas, ab)]


def compare(got, want, what):
    """The same zero pattern and rtol = 2e-6; returns the largest relative difference."""
    assert got.shape == want.shape and got.dtype == np.float32, what
    assert np.array_equal(got != 0, want != 0), what
    assert np.allclose(got, want, rtol=RTOL, atol=0), what
    nz = want != 0
    return float(np.max(np.abs(got[nz].astype(np.float64) - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0
