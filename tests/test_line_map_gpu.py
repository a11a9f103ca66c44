"""mcgpu_line_map on the device against the restatement over the oracle's operators (tests/line_walk.py): the cases and the
comparison of tests/test_line_map.py (rtol 2e-6, atol 1e-8 x the cube's largest value, the same zero pattern, n_capped == 0),
repeated calls, the two known answers that catch a wrong lane-to-channel mapping (far wings, channel subsets), method 1, the
host pipeline's shapes and the refusals."""
import numpy as np
import pytest

import line_cases as L
import line_walk as W
from mcfost_amd.host import molecule as MOL

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 3, 5     # MCGPU_ERR_ARG, MCGPU_ERR_STATE (include/mcgpu.h)
MAX_CHANNELS = 1024           # MCGPU_LINE_MAX_CHANNELS


@pytest.fixture(scope="module")
def engine():
    """One engine per grid for the whole module (mcgpu_line_map keeps nothing in the context)."""
    from mcfost_amd.engine import Engine
    made = {}

    def get(grid):
        if grid not in made:
            made[grid] = Engine(L.grid_case(grid)[0], 1000)
        return made[grid]

    yield get
    for e in made.values():
        e.close()


def image(e, m, mol, **kw):
    return e.line_map(mol, method=2, npix_x=L.NPIX, npix_y=L.NPIX, map_size=L.map_size(m), **kw)


@pytest.mark.parametrize("n_speed", L.N_SPEEDS)
@pytest.mark.parametrize("name", list(L.CASES))
def test_device_against_the_restatement(engine, name, n_speed):
    m, _, mol, want = L.case(name, n_speed)
    e = engine(L.CASES[name][0])
    spec, cont, capped, ms = image(e, m, mol)
    assert capped == 0 and ms > 0.0
    worst = max(L.compare(spec, want["spectrum"], (name, "spectrum")), L.compare(cont, want["continu"], (name, "continu")))
    print("%s n_speed %d: largest relative difference to the restatement %.3g, %.3f ms" % (name, n_speed, worst, ms))
    # a second call: identical bits (no atomics in the sums)
    spec2, cont2, capped2, _ = image(e, m, mol)
    assert capped2 == 0
    assert np.array_equal(spec2.view(np.uint32), spec.view(np.uint32)) and np.array_equal(cont2.view(np.uint32), cont.view(np.uint32))
    # one output alone
    only, none, _, _ = image(e, m, mol, continu=False)
    assert none is None and np.array_equal(only.view(np.uint32), spec.view(np.uint32))


@pytest.mark.parametrize("name", ["cyl2d", "voronoi"])
def test_far_wings_equal_the_continuum_bit_for_bit(engine, name):
    """Channels 0 and 34 lie where the profile is exactly 0; with 81 + 2 channels they sit in lane 0 of the first pass and lane
    18 of the second."""
    m = L.grid_case(L.CASES[name][0])[0]
    e = engine(L.CASES[name][0])
    for n in (33, 81):
        ts = np.concatenate([[-4.0e7], MOL.tab_speed_rt(-L.VMAX, L.VMAX, n), [4.0e7]])
        mol = L.tables(name, n + 2, tab_speed=ts)
        spec, cont, capped, _ = image(e, m, mol)
        assert capped == 0 and (cont > 0).sum() > 10
        for iv in (0, n + 1):
            assert np.array_equal(spec[:, :, iv].view(np.uint32), cont.view(np.uint32)), (n, iv)
        assert not np.array_equal(spec[:, :, (n + 1) // 2], cont)


@pytest.mark.parametrize("name", ["cyl2d", "cyl3d"])
def test_channel_subsets_give_the_same_bits(engine, name):
    m, _, mol, _ = L.case(name, 81)
    e = engine(L.CASES[name][0])
    pick = np.array([0, 3, 7, 16, 17, 31, 40, 41, 50, 62, 63, 64, 65, 70, 77, 79, 80])
    sub = L.tables(name, 17, tab_speed=np.asarray(mol["tab_speed"])[pick])
    full = image(e, m, mol)[0]
    part = image(e, m, sub)[0]
    assert np.array_equal(part.view(np.uint32), full[:, :, pick].view(np.uint32))


def test_method1(engine):
    name = "cyl2d"
    m, o, _, _, _ = L.grid_case(name)
    e = engine(name)
    mol = L.tables(name, 33)
    rays = W.ray_starts(m, 1)
    want = W.cube_from_paths(m, mol, rays, W.walk_paths(o, m, rays))
    spec, cont, capped, ms = e.line_map(mol, method=1)
    assert capped == 0 and spec.shape == (2, 2, 33, 1, 1) and cont.shape == (2, 2, 1, 1)
    print("method 1: largest relative difference %.3g, %.3f ms" % (
        max(L.compare(spec, want["spectrum"], "method 1 spectrum"), L.compare(cont, want["continu"], "method 1 continu")), ms))
    again = e.line_map(mol, method=1)
    assert np.array_equal(again[0].view(np.uint32), spec.view(np.uint32)) and np.array_equal(again[1].view(np.uint32), cont.view(np.uint32))


@pytest.mark.parametrize("name", ["cyl2d", "cyl3d"])
def test_pipeline_shapes(engine, name):
    from mcfost_amd.host import pipeline as P
    m, _, mol, _ = L.case(name, 33)
    e = engine(L.CASES[name][0])
    n_incl, n_az = m.rt["RT_n_incl"], m.rt["RT_n_az"]
    spec, cont = P.line_map(P.EngineBackend(e), m, mol, npix_x=L.NPIX, npix_y=7, map_size=L.map_size(m))
    assert spec.shape == (n_az, n_incl, 2, 33, 7, L.NPIX) and cont.shape == (n_az, n_incl, 2, 7, L.NPIX)
    assert spec.dtype == np.float32 and cont.dtype == np.float32
    flat = e.line_map(mol, npix_x=L.NPIX, npix_y=7, map_size=L.map_size(m))[0]
    assert np.array_equal(spec.reshape(flat.shape), flat)
    s1, c1 = P.line_map(P.EngineBackend(e), m, mol, method=1)
    assert s1.shape == (n_az, n_incl, 2, 33, 1, 1) and c1.shape == (n_az, n_incl, 2, 1, 1) and (s1 > 0).all()
    # l_sym_ima: the columns beyond npix_x / 2 + mod(npix_x, 2) stay 0
    sym = e.line_map(mol, npix_x=L.NPIX, npix_y=7, map_size=L.map_size(m), l_sym_ima=True)[0]
    assert np.array_equal(sym[..., :L.NPIX // 2], flat[..., :L.NPIX // 2]) and not sym[..., L.NPIX // 2:].any()


def test_refusals(engine):
    from mcfost_amd.engine import Engine, McgpuError
    name = "cyl2d"
    m = L.grid_case(name)[0]
    e = engine(name)

    def refused(eng, mm, code, mol, **kw):
        with pytest.raises(McgpuError) as err:
            eng.line_map(mol, npix_x=4, npix_y=4, map_size=L.map_size(mm), **kw)
        assert err.value.code == code, str(err.value)

    # n_speed * nTrans over the cap
    n = MAX_CHANNELS // 2 + 1
    refused(e, m, ERR_ARG, L.tables(name, n, tab_speed=np.linspace(-L.VMAX, L.VMAX, n)))
    # a NULL array that the mode needs
    for key in ("dv_line", "vfield", "kappa_mol_o_freq", "emissivite_dust", "norme_phiProf_m1"):
        mol = L.tables(name, 33)
        mol[key] = None
        refused(e, m, ERR_ARG, mol)
    mol = L.tables(name, 33)
    mol["lkeplerian"] = False
    refused(e, m, ERR_ARG, mol)                                   # an analytic field that is neither Keplerian nor infall
    refused(e, m, ERR_ARG, L.tables(name, 33), method=3)
    mol = L.tables("sph2d", 33)
    mol["vfield_coord"] = 4
    refused(engine("sph2d"), L.grid_case("sph2d")[0], ERR_ARG, mol)
    # a Voronoi grid without vxyz
    mv = L.grid_case("voronoi")[0]
    mol = L.tables("voronoi", 33)
    mol["vxyz"] = None
    refused(engine("voronoi"), mv, ERR_ARG, mol)
    # the context is as usable as before
    assert e.line_map(L.tables(name, 33), npix_x=4, npix_y=4, map_size=L.map_size(m))[2] == 0
    # a context without opacities: the grid alone
    b = Engine.bare()
    b.model = m
    b._upload_grid_cyl(m)
    b._rt1 = True                                                 # (no observers either: the call itself must refuse)
    refused(b, m, ERR_STATE, L.tables(name, 33))
    b.close()


def test_fortran_shim_has_the_interface():
    import os
    import __graft_entry__ as g
    assert os.path.exists("/opt/rocm/bin/amdflang"), "no Fortran compiler: the shim's interfaces cannot be checked"
    mod = os.path.join(g.ROOT, "mcfost_amd", "fortran", "build", "mcgpu_f.o")
    if os.path.exists(mod):
        os.remove(mod)
    g.build_fortran_shim()
    assert os.path.exists(mod)
    src = open(os.path.join(g.ROOT, "mcfost_amd", "fortran", "mcgpu_f.f90")).read()
    assert 'bind(C, name="mcgpu_line_map")' in src and "mcgpu_line_opts" in src
