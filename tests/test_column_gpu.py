"""mcgpu_compute_column / mcgpu_integ_tau on the device against the walk over the oracle's operators (tests/column_walk.py):
the five grids, types and tolerance of tests/test_column.py (rtol = 2e-6, the same zero pattern, n_capped == 0), repeated
calls, variable dust, the host pipeline's shapes and the refusals."""
import copy

import numpy as np
import pytest

import column_cases as K
import column_walk as W
from mcfost_amd.host import model as M

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 3, 5     # MCGPU_ERR_ARG, MCGPU_ERR_STATE (include/mcgpu.h)
ANGLE = 80.0                  # integ_tau: degrees from the axis, a ray inside the flared disk


@pytest.mark.parametrize("name", list(K.GRIDS))
def test_device_against_the_walk(name):
    from mcfost_amd.engine import Engine
    m, _, paths = K.case(name)
    e = Engine(m, 1000)
    worst = 0.0
    for type, lam, gas, ab in K.variants(m):
        want = W.column_from_paths(paths, W.factor_of(m, type, lam, gas, ab))
        got, capped, ms = e.compute_column(type, lam=lam, gas_density=gas, abundance=ab)
        assert capped == 0 and ms > 0.0
        worst = max(worst, K.compare(got, want, (name, type, lam)))
        # a second call with the same arguments: identical bits (one ray per lane, no atomics in the sums)
        again, capped2, _ = e.compute_column(type, lam=lam, gas_density=gas, abundance=ab)
        assert capped2 == 0 and np.array_equal(again.view(np.uint32), got.view(np.uint32))
    print("%s: largest relative difference to the walk %.3g" % (name, worst))
    e.close()


@pytest.mark.parametrize("name", ["cyl2d", "sph3d", "voronoi"])
def test_variable_dust(name):
    from mcfost_amd.engine import Engine
    m, _, paths = K.case(name)
    l1, l2 = K.wavelengths(m)
    e = Engine(m, 1000)
    single = {lam: e.compute_column(2, lam=lam)[0] for lam in (l1, l2)}
    e.close()
    # every class equal to the model's tables: the single-class result bit for bit
    mi = copy.copy(m)
    M.init_variable_dust(mi, identical=True)
    e = Engine(mi, 1000)
    for lam in (l1, l2):
        got, capped, _ = e.compute_column(2, lam=lam)
        assert capped == 0 and np.array_equal(got.view(np.uint32), single[lam].view(np.uint32)), lam
    e.close()
    # distinct classes: the class of the current cell
    mv = copy.copy(m)
    M.init_variable_dust(mv)
    e = Engine(mv, 1000)
    for lam in (l1, l2):
        want = W.column_from_paths(paths, W.factor_of(mv, 2, lam))
        got, capped, _ = e.compute_column(2, lam=lam)
        assert capped == 0
        K.compare(got, want, (name, "variable dust", lam))
        assert not np.allclose(got, single[lam], rtol=1e-3)
    e.close()


@pytest.mark.parametrize("name", ["cyl2d", "cyl3d", "sph2d", "voronoi"])
def test_integ_tau(name):
    from mcfost_amd.engine import Engine
    from mcfost_amd.host import pipeline as P
    m, o, _ = K.case(name)
    e = Engine(m, 1000)
    for lam in K.wavelengths(m):
        want = W.integ_tau_walk(o, m, lam, ANGLE)
        got = e.integ_tau(lam, ANGLE)
        assert want[0] > 0 and want[1] > 0
        assert np.allclose(got, want, rtol=K.RTOL, atol=0), (name, lam, got, want)
        r = P.integ_tau(P.EngineBackend(e), m, lam, ANGLE)
        assert r["tau_midplane"] == got[0] and r["tau_angle"] == got[1]
        # the column densities printed next to them (optical_depth.f90:216-221): tau x rho / (kappa kappa_factor / AU_to_cm)
        i = m.extra["icell_ref"] - 1
        cd = float(got[0]) * m.rho_dust[i] / (m.kappa[lam - 1] * m.kappa_factor[i] / M.AU_TO_CM)
        assert np.isclose(float(r["column_midplane"]), cd, rtol=1e-6)
    e.close()


@pytest.mark.parametrize("name", ["cyl2d", "cyl3d", "voronoi"])
def test_pipeline_column_maps(name):
    from mcfost_amd.engine import Engine
    from mcfost_amd.host import pipeline as P
    m, _, _ = K.case(name)
    e = Engine(m, 1000)
    lam = K.wavelengths(m)[1]
    gas, ab = K.seeded(m)
    g = m.grid
    shape = (4, m.n_cells) if name == "voronoi" else ((4, g["n_az"], 2 * g["nz"], g["n_rad"]) if g["l3D"] else (4, g["nz"], g["n_rad"]))
    for type, kw in ((1, dict(gas_density=gas)), (2, dict(lam=lam)), (3, dict(gas_density=gas, abundance=ab))):
        flat = e.compute_column(type, **kw)[0]
        maps = P.column_maps(P.EngineBackend(e), m, type, **kw)
        assert maps.shape == shape and maps.dtype == np.float32
        assert np.array_equal(maps.reshape(4, -1), flat)              # the flat order is the engine's: icell fastest
    if name == "cyl2d":    # (i, j) of the file = (radius, layer): the optical depth towards +z falls with the layer
        tz = P.column_maps(P.EngineBackend(e), m, 2, lam=lam)[1]
        assert np.all(np.diff(tz, axis=0) < 0)
    e.close()


def test_refusals():
    from mcfost_amd.engine import Engine, McgpuError
    m, _, _ = K.case("cyl2d")
    gas, ab = K.seeded(m)
    e = Engine(m, 1000)

    def refused(code, *a, **kw):
        with pytest.raises(McgpuError) as err:
            e.compute_column(*a, **kw)
        assert err.value.code == code, str(err.value)

    refused(ERR_ARG, 0, lam=3, gas_density=gas, abundance=ab)
    refused(ERR_ARG, 4, lam=3, gas_density=gas, abundance=ab)
    refused(ERR_ARG, 2, lam=0)
    refused(ERR_ARG, 2, lam=m.n_lambda + 1)
    refused(ERR_ARG, 1)                                   # type 1 without gas_density
    refused(ERR_ARG, 3, gas_density=gas)                  # type 3 without abundance
    for lam in (0, m.n_lambda + 1):
        with pytest.raises(McgpuError) as err:
            e.integ_tau(lam, 45.0)
        assert err.value.code == ERR_ARG
    # the context is as usable as before
    assert e.compute_column(2, lam=3)[1] == 0
    e.close()
    # a context without opacities: the grid alone
    e = Engine.bare()
    e.model = m
    e._upload_grid_cyl(m)
    refused(ERR_STATE, 2, lam=3)
    with pytest.raises(McgpuError) as err:
        e.integ_tau(3, 45.0)
    assert err.value.code == ERR_STATE
    e.close()


def test_fortran_shim_compiles():
    """The ISO_C_BINDING module with the two new interface blocks goes through the Fortran compiler (the library's machines
    have one: its absence is a failure here, not a pass)."""
    import os
    import __graft_entry__ as g
    assert os.path.exists("/opt/rocm/bin/amdflang"), "no Fortran compiler: the shim's interfaces cannot be checked"
    mod = os.path.join(g.ROOT, "mcfost_amd", "fortran", "build", "mcgpu_f.o")
    if os.path.exists(mod):
        os.remove(mod)
    g.build_fortran_shim()
    assert os.path.exists(mod)
    src = open(os.path.join(g.ROOT, "mcfost_amd", "fortran", "mcgpu_f.f90")).read()
    assert 'bind(C, name="mcgpu_compute_column")' in src and 'bind(C, name="mcgpu_integ_tau")' in src
